"""Pins the fp64 references of the flow's element training operators (tests/elem_ops_ref.py) to the oracle, checks on the CPU that the
inputs committed for the GPU tests (tests/test_gpu_train_elem_ops.py) decide every clamp and keep every matrix norm on its side of the
narrow ExponentialCoupling kernel's bound (csrc/train_expm.hip), and measures the yardstick of that kernel's gate."""
import math

import pytest
import torch

import elem_ops_ref as R
from oracle import flow_oracle as O

TOL = 1e-12


def _close(a, b):
    return R.rel(a, b) < TOL


@pytest.mark.parametrize("kind", ["exp", "sigmoid"])
def test_affine_ref_equals_the_oracle_affine_coupling_lines(kind):
    g = torch.Generator().manual_seed(0)
    rows, d2 = 7, 5
    b, st = torch.randn(rows, d2, generator=g, dtype=torch.float64), 1.5 * torch.randn(rows, 2 * d2, generator=g, dtype=torch.float64)
    s = O._affine_scale(st[..., :d2], kind)
    t = st[..., d2:]
    y2, ldj = R.affine_ref(b, st, d2, kind)
    assert _close(y2, b * s + t) and _close(ldj, torch.log(s).sum(-1))


def _oracle_scale(p, nz, clamp):
    """as cond_normal_params produces it: exp, then clamp_max"""
    scale = p[..., nz:].exp()
    if clamp:
        scale = scale.clamp_max(clamp)
    return p[..., :nz], scale


@pytest.mark.parametrize("name", ["g300_n150_c10", "g300_n3_c05_wide", "g300_n32_c0"])
def test_gauss_draw_ref_equals_the_oracle_normal(name):
    c = R.make_gauss_case(name)
    nz, p, eps = c["nz"], c["p"].double(), c["eps"].double()
    mean, scale = _oracle_scale(p, nz, c["clamp"])
    z, ldj = R.gauss_draw_ref(p, eps, nz, c["clamp"])
    assert _close(z, mean + eps * scale) and _close(ldj, -O.normal_log_prob(mean + eps * scale, mean, scale).sum(-1))


@pytest.mark.parametrize("name", ["l300_n150_c10", "l1_n3_c05", "l300_n32_c0"])
def test_normal_log_prob_ref_equals_the_oracle_normal(name):
    c = R.make_normlp_case(name)
    nz, p, v = c["nz"], c["p"].double(), c["v"].double()
    mean, scale = _oracle_scale(p, nz, c["clamp"])
    assert _close(R.normal_log_prob_ref(v, p, nz, c["clamp"]), O.normal_log_prob(v, mean, scale).sum(-1))


def test_base_density_ref_equals_the_oracle_standard_normal():
    x = R.make_base_case("b300_w300_u30_wide")["x"].double()
    assert _close(R.base_density_ref(x), O.std_normal_log_prob(x))


def test_act_ref_equals_torch():
    u = 3 * torch.randn(50, 7, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    F = torch.nn.functional
    for name, fn in (("GELU", F.gelu), ("RELU", F.relu), ("ELU", F.elu)):
        assert _close(R.act_ref(u, name), fn(u))


@pytest.mark.parametrize("table,name", R.clamp_cases())
def test_committed_clamp_inputs_are_decided_and_clamp_gradients_follow_autograd(table, name):
    """Every log std at least 1e-3 from log(clamp), at least a quarter of them on either side; the reference's log-std gradient equals
    fp64 autograd through the oracle's exp -> clamp_max and is exactly zero where clamped (dldj / g carry no part of it there)."""
    c = R.make_gauss_case(name) if table == "gauss" else R.make_normlp_case(name)
    nz, clamp = c["nz"], c["clamp"]
    margin, above, below = R.clamp_margins(c)
    print(f"{name}: min |log std - log clamp| {margin:.2e}  share above {above:.3f} below {below:.3f}")
    assert margin >= R.CLAMP_MARGIN and above >= R.CLAMP_SHARE and below >= R.CLAMP_SHARE
    r = (R.gauss_refs if table == "gauss" else R.normlp_refs)(c, torch.float64)
    p = c["p"].double().requires_grad_(True)
    mean, scale = _oracle_scale(p, nz, clamp)
    if table == "gauss":
        z = mean + c["eps"].double() * scale
        L = (z * c["dz"].double()).sum() - (O.normal_log_prob(z, mean, scale).sum(-1) * c["dldj"].double()).sum()
    else:
        L = (O.normal_log_prob(c["v"].double(), mean, scale).sum(-1) * c["g"].double()).sum()
    L.backward()
    assert _close(r["dmean"], p.grad[:, :nz]) and _close(r["dlogstd"], p.grad[:, nz:])
    clamped = c["p"][:, nz:].double() > math.log(clamp)
    assert clamped.any() and (~clamped).any()
    assert (r["dlogstd"][clamped] == 0).all() and (r["dlogstd"][~clamped] != 0).all()


@pytest.mark.parametrize("name", list(R.EXPM_CASES))
def test_committed_expm_inputs_stay_below_the_norm_bound(name):
    c = R.make_expm_case(name)
    nrm = R.expm_w(c["raw"], c["scal4"], torch.float64).abs().sum(-1).max(-1).values
    print(f"{name}: |W|_inf {nrm.min().item():.3g} .. {nrm.max().item():.3g}")
    assert (nrm <= 0.9 * R.EXPM_NORM_LIMIT).all()


def test_the_bound_case_exceeds_the_norm_bound_in_every_row():
    c = R.make_expm_case("bound")
    nrm = R.expm_w(c["raw"], c["scal4"], torch.float64).abs().sum(-1).max(-1).values
    assert (nrm > R.EXPM_NORM_LIMIT).all()


def test_narrow_recurrence_in_fp32_against_fp64_autograd():
    """The yardstick of the narrow ExponentialCoupling gate: elem_ops_ref.narrow_recurrence_backward in fp32 on the fp32 W of every
    committed case against fp64 autograd through torch.matrix_exp, per tensor max |a - a64| / max |a64|.  Measured (the host's
    summation order may move the last digit): y 2.7e-8 .. 7.3e-7, dx 2.7e-8 .. 2.0e-7, dW 4.5e-8 .. 1.4e-6; the largest, 1.4e-6 (dW of
    x1_n16_r70: one scalar W = 16 per point, s = 5, exp(16) = 8.9e6), makes the GPU gate max(2e-6, 3 x 1.4e-6) = 4.2e-6.  s takes the
    values 0 (||W||_1 = 0.01), 0 .. 1 (0.3), 3 .. 4 (4.0) and 5 .. 6 (16.0); in fp64 the same restatement is within 1e-12 of
    torch.matrix_exp: the recurrence is the function, its fp32 error is rounding."""
    seen = set()
    for name, (ey, ex, ew, s0, s1) in R.narrow_yardstick().items():
        print(f"{name}: s {s0}..{s1}  y {ey:.1e} dx {ex:.1e} dW {ew:.1e}")
        assert max(ey, ex, ew) < 5e-6                                    # rounding, not algebra: an fp32 restatement that is wrong is off by 1e-2
        seen.update(range(s0, s1 + 1))
    assert seen >= {0, 1, 3, 4, 5, 6}                                    # (s = 2 needs 1 < |W|_inf <= 2, between the norms 0.3 and 4.0)
    print(f"gate of the narrow kernels: {R.expm_gate():.2e}")
    assert 2e-6 <= R.expm_gate() < 1.5e-5
    # the same restatement in fp64: the truncation after 12 terms at |A|_inf <= 1/2 is below 1e-12
    c = R.make_expm_case("x16_n16_r70")
    W = R.expm_w(c["raw"], c["scal4"], torch.float64).requires_grad_(True)
    x = c["x2"].double().requires_grad_(True)
    y64 = torch.einsum("rij,rj->ri", torch.matrix_exp(W), x)
    (y64 * c["dy2"].double()).sum().backward()
    y, dx, dW, _ = R.narrow_recurrence_backward(W.detach(), x.detach(), c["dy2"].double())
    assert R.rel(y, y64.detach(), 0.0) < 1e-12 and R.rel(dx, x.grad, 0.0) < 1e-12 and R.rel(dW, W.grad, 0.0) < 1e-12
    # one point alone equals the same point in the batch
    W32 = R.expm_w(c["raw"], c["scal4"], torch.float32)
    yb, dxb, dWb, sb = R.narrow_recurrence_backward(W32, c["x2"], c["dy2"])
    y1, dx1, dW1, s1 = R.narrow_recurrence_backward(W32[3], c["x2"][3], c["dy2"][3])
    assert s1 == int(sb[3]) and torch.allclose(y1, yb[3], rtol=1e-5, atol=0) and torch.allclose(dW1, dWb[3], rtol=1e-4, atol=1e-6)
