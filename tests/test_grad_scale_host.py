"""CPU side of the upstream-gradient-scale tests: the premises of test_gpu_train_grad_scale.py, checked without a GPU.
(a) the fp64 reference scales exactly with 2^e and the scaled input is an exact, normal fp32 number; (b) an eager fp32 restatement
of the same backward meets the GPU tests' gate at every case and exponent, so the gate is reachable in fp32 arithmetic; (c) the
emulated fixed-scale limb split misses the gate for attention at e <= -14: why the GPU test exists."""
import numpy as np
import pytest
import torch

import grad_scale_util as U

ATTENTION_RUNS = ([(c, e) for c in U.SCALED_CASES for e in U.EXPONENTS] + [(c, e) for c in U.CONTROL_CASES for e in U.CONTROL_EXPONENTS]
                  + [("range", e) for e in U.RANGE_EXPONENTS] + [U.TWO_SCALE])
LINEAR_RUNS = [(c, e) for c in U.LINEAR_CASES for e in U.LINEAR_GATED_EXPONENTS + U.LINEAR_REPORTED_EXPONENTS]
FP32_TINY = float(np.finfo(np.float32).tiny)


def _exact_normal_fp32(t):
    nz = t[t != 0]
    return bool((t.float().double() == t).all()) and bool((nz.abs() >= FP32_TINY).all()) and bool(torch.isfinite(t.float()).all())


@pytest.mark.parametrize("case,e", ATTENTION_RUNS)
def test_attention_reference_scales_exactly_and_the_scaled_input_is_exact_in_fp32(case, e):
    es = U.exponents_of(case, e)
    base, ref = U.scaled_reference(case, 0), U.scaled_reference(case, e)
    f = torch.tensor([2.0 ** x for x in es], dtype=torch.float64)[:, None, None]
    for n in ("dq", "dk", "dv"):
        assert torch.equal(ref[n], base[n] * f), (case, e, n)
    assert torch.equal(ref["out"], base["out"])
    assert _exact_normal_fp32(U.scaled_dout(case, e))


@pytest.mark.parametrize("case,e", LINEAR_RUNS)
def test_linear_reference_scales_exactly_and_the_scaled_input_is_exact_in_fp32(case, e):
    base, ref = U.linear_reference(case, 0), U.linear_reference(case, e)
    for n in base:
        assert torch.equal(ref[n], base[n] * (1.0 if n == "y" else 2.0 ** e)), (case, e, n)
    assert _exact_normal_fp32(U.linear_inputs(case)[4] * 2.0 ** e)


@pytest.mark.parametrize("case,e", ATTENTION_RUNS)
def test_eager_fp32_attention_backward_meets_the_gate(case, e):
    q, k, v, _, scale = U.attention_inputs(case)
    got = U.attention_backward(q.float(), k.float(), v.float(), U.scaled_dout(case, e).float(), scale)
    errs = U.attention_errors(case, e, got)
    assert max(errs.values()) < U.GATE, errs


@pytest.mark.parametrize("case,e", LINEAR_RUNS)
def test_eager_fp32_linear_backward_meets_the_gate(case, e):
    W, b, xs, r, dy = U.linear_inputs(case)
    got = U.linear_backward(W.float(), b.float(), [x.float() for x in xs], None if r is None else r.float(), (dy * 2.0 ** e).float(),
                            U.LINEAR_CASES[case]["act"])
    errs = U.linear_errors(case, e, got)
    assert max(errs.values()) < U.GATE, errs


def test_range_case_overflows_fp16_in_dS_only():
    """Every operand of the range case is far inside the fp16 range; dS = P (dP - D) scale is not."""
    q, k, v, dout, scale = U.attention_inputs("range")
    assert max(t.abs().max().item() for t in (q, k, v, dout)) < 65504.0 / 2
    p = torch.softmax(q @ k.transpose(1, 2) * scale, -1)
    ds = p * (dout @ v.transpose(1, 2) - (dout * (p @ v)).sum(-1, keepdim=True)) * scale
    assert ds.abs().max().item() > 65504.0 and p.max().item() > 0.9
    assert (U.scaled_dout("range", 15).abs().max().item()) > 65504.0


def test_one_key_softmax_owes_exact_zeros():
    ref = U.scaled_reference("one_key", 0)
    assert ref["dq"].abs().max().item() == 0.0 and ref["dk"].abs().max().item() == 0.0


def test_scene_error_judges_each_scene_against_its_own_scale():
    ref = torch.stack([torch.ones(4, 4), torch.full((4, 4), 2.0 ** -20)]).double()
    got = ref.clone()
    got[1] *= 1.5                                                   # 50 % wrong, invisible beside scene 0
    assert (got - ref).abs().max().item() / ref.abs().max().item() < U.GATE
    assert U.scene_error(got, ref, 1e-2, (0, -20)) == pytest.approx(0.5)
    got[1, 0, 0] = float("nan")
    assert U.scene_error(got, ref, 1e-2, (0, -20)) == float("inf")


def test_limb_split_rounds_like_fp16_with_subnormals():
    hi, lo = U.limb_split(np.float32([1.0 + 2.0 ** -12, 2.0 ** -25, 3e-8, 7e4, 0.0]))
    assert hi[0] == 1.0 and lo[0] == 0.5                             # (x - hi) 2048 = 2^-12 2^11
    assert hi[1] == 0.0 and lo[1] == 2.0 ** -14                      # below half the smallest subnormal: hi is zero, lo' keeps one bit
    assert hi[2] == 2.0 ** -24                                       # a subnormal hi
    assert np.isinf(hi[3]) and hi[4] == 0.0 and lo[4] == 0.0


@pytest.mark.parametrize("e", U.EXPONENTS)
def test_emulated_fixed_scale_split_misses_the_gate_for_small_gradients(e):
    """The fixed-scale split of dS = P (dP - D) scale: P ~ 1e-3, so at dout ~ 2^-14 the hi limb is subnormal and lo' holds few bits."""
    errs = U.attention_errors("long_diffuse", e, U.emulated_attention_backward("long_diffuse", e))
    print(f"emulated long_diffuse e {e}: " + " ".join(f"{n} {x:.1e}" for n, x in errs.items()))
    if e == 0:
        assert max(errs.values()) < U.GATE, errs
    if e <= -14:
        assert max(errs["dq"], errs["dk"]) > U.GATE, errs
