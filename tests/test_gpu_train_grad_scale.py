"""The training backward kernels across upstream-gradient scales.  Every other operator test feeds the backward a `randn` gradient
(magnitude 1); a training step's gradient of a mean over all points is ~1e-5 and smaller.  A backward is linear in its upstream
gradient, so dout 2^e must give the fp64 reference's gradients times 2^e under the operator tests' own gate with its floors times
2^e (grad_scale_util.py; the premises are checked on the CPU in test_grad_scale_host.py)."""
import ctypes

import pytest
import torch

from flowcompare_amd import engine
from flowcompare_amd import train_ops as T
import grad_scale_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _attention(case, e, fp16, scenes=None):
    """T.attention forward + backward on panels under a step guard -> (out, dq, dk, dv as [B, ., I] on the host; range flag)."""
    q, k, v, _, scale = U.attention_inputs(case)
    dout = U.scaled_dout(case, e)
    if scenes is not None:
        q, k, v, dout = (t[scenes] for t in (q, k, v, dout))
    B, N, I = q.shape
    M = k.shape[1]
    qd, kd, vd = (t.float().to(DEV).requires_grad_(True) for t in (q, k, v))
    with T.step_guard(fp16=fp16, device=DEV) as guard:
        op = T.attention(T.to_panel(qd.reshape(B * N, I)), T.to_panel(kd.reshape(B * M, I)), T.to_panel(vd.reshape(B * M, I)), B, N, M, scale)
        o = T.from_panel(op, B * N, I).reshape(B, N, I)
        o.backward(dout.float().to(DEV))
        flagged = guard.overflowed()
    return dict(out=o.detach().cpu(), dq=qd.grad.cpu(), dk=kd.grad.cpu(), dv=vd.grad.cpu()), flagged


def _report(what, errs):
    print(what + ": " + " ".join(f"{n} {x:.1e}" for n, x in errs.items()))


@pytest.mark.parametrize("e", U.EXPONENTS)
@pytest.mark.parametrize("case", U.SCALED_CASES)
def test_attention_backward_holds_its_gate_at_every_gradient_scale(case, e):
    got, flagged = _attention(case, e, fp16=True)
    errs = U.attention_errors(case, e, got)
    _report(f"attention {case} e {e} fp16 True", errs)
    assert not flagged
    assert max(errs.values()) < U.GATE, errs
    if case == "one_key":                                             # O = v, dP = D: the zeros are owed exactly, at every scale
        assert got["dq"].abs().max().item() == 0.0 and got["dk"].abs().max().item() == 0.0


@pytest.mark.parametrize("e", U.CONTROL_EXPONENTS)
@pytest.mark.parametrize("case,fp16", [(c, False) for c in U.SCALED_CASES] + [(c, f) for c in U.CONTROL_CASES for f in (True, False)])
def test_fp32_input_attention_kernels_hold_the_gate_at_both_scales(case, fp16, e):
    """Controls: the guard off, and head dims 32 and 128, run on the fp32-input kernels, which split nothing."""
    got, flagged = _attention(case, e, fp16=fp16)
    errs = U.attention_errors(case, e, got)
    _report(f"attention control {case} e {e} fp16 {fp16}", errs)
    assert not flagged
    assert max(errs.values()) < U.GATE, errs


def test_two_scenes_at_different_gradient_scales_are_each_held_to_their_own():
    """The grid's y index is the scene and no contraction crosses scenes: scene 1 at 2^-20 is judged at 2^-20, beside scene 0 at 1."""
    case, es = U.TWO_SCALE
    got, flagged = _attention(case, es, fp16=True)
    errs = U.attention_errors(case, es, got)
    _report(f"attention {case} e {es} fp16 True", errs)
    assert not flagged
    assert max(errs.values()) < U.GATE, errs


@pytest.mark.parametrize("e", U.CONTROL_EXPONENTS)
@pytest.mark.parametrize("stats_valid", [1, 0])
def test_both_log_sum_exp_paths_of_the_dq_kernel(stats_valid, e):
    """have_lse = 1 takes the forward's saved statistics, have_lse = 0 (stats_valid = 0) runs the dq kernel's own log-sum-exp pass."""
    case = "two_wg_diffuse"
    q, k, v, _, scale = U.attention_inputs(case)
    B, N, I = q.shape
    M = k.shape[1]
    L = engine.lib()
    qp, kp, vp = (T.to_panel(t.float().reshape(-1, I)).to(DEV) for t in (q, k, v))           # row-padded panels, as AttentionFn passes them
    dout = T.to_panel(U.scaled_dout(case, e).float().reshape(-1, I)).to(DEV)
    out = torch.zeros_like(qp)
    dq, dk, dv = torch.full_like(qp, float("nan")), torch.full_like(kp, float("nan")), torch.full_like(vp, float("nan"))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    stats = torch.empty(2 * B * N, dtype=torch.float32, device=DEV)
    nb = L.fc_train_attention_ws_bytes(B, N, M, I)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    valid = ctypes.c_int32(0)
    L.fc_train_attention_fwd_f32(engine._ptr(qp), I, engine._ptr(kp), I, engine._ptr(vp), I, engine._ptr(out), I, B, N, M, I, scale, engine._ptr(ws), nb,
                                 engine._ptr(stats), ctypes.byref(valid), engine._ptr(flag), engine._stream())
    assert valid.value == 1
    if not stats_valid:
        stats.fill_(float("nan"))                                     # nothing of the forward's statistics may be read
    L.fc_train_attention_bwd_f32(engine._ptr(qp), I, engine._ptr(kp), I, engine._ptr(vp), I, engine._ptr(out), I, engine._ptr(dout), I, engine._ptr(dq), I,
                                 engine._ptr(dk), I, engine._ptr(dv), I, engine._ptr(stats), stats_valid, B, N, M, I, scale, engine._ptr(flag), engine._stream())
    torch.cuda.synchronize()
    got = dict(out=out[:B * N].reshape(B, N, I).cpu(), dq=dq[:B * N].reshape(B, N, I).cpu(), dk=dk[:B * M].reshape(B, M, I).cpu(),
               dv=dv[:B * M].reshape(B, M, I).cpu())
    errs = U.attention_errors(case, e, got)
    _report(f"attention {case} e {e} stats_valid {stats_valid}", errs)
    assert flag.item() == 0
    assert max(errs.values()) < U.GATE, errs


@pytest.mark.parametrize("e", U.RANGE_EXPONENTS)
def test_attention_backward_range_contract(e):
    """Operands far inside the fp16 range whose dS = P (dP - D) scale is not (and, at e = 15, a dout outside it): either the gradients are
    finite and meet the gate, or the range flag is up and the fp32-input repeat meets it.  Wrong gradients under a clear flag are the failure."""
    got, flagged = _attention("range", e, fp16=True)
    errs = U.attention_errors("range", e, got)
    _report(f"attention range e {e} fp16 True flagged {flagged}", errs)
    if max(errs.values()) < U.GATE:
        return
    assert flagged, errs
    again, flagged32 = _attention("range", e, fp16=False)
    errs32 = U.attention_errors("range", e, again)
    _report(f"attention range e {e} fp16 False", errs32)
    assert not flagged32 and max(errs32.values()) < U.GATE, errs32


def test_a_scene_alone_gives_the_bytes_it_gives_inside_a_batch():
    """Scene 1 of two, run alone: the same bytes of dq, dk and dv (the scene offsets of the log-sum-exp and D vectors, and of whatever
    the kernels derive per scene)."""
    case, es = U.TWO_SCALE
    both, _ = _attention(case, es, fp16=True)
    alone, _ = _attention(case, es, fp16=True, scenes=slice(1, 2))
    for n in ("dq", "dk", "dv"):
        assert torch.equal(both[n][1], alone[n][0]), n


# ---------------------------------------------------------------- Linear
def _linear(case, e, fp16=True):
    c = U.LINEAR_CASES[case]
    rows, widths, N, act = c["rows"], list(c["widths"]), c["N"], c["act"]
    W, b, xs, r, dy = U.linear_inputs(case)
    Wd, bd = W.float().to(DEV).requires_grad_(True), b.float().to(DEV).requires_grad_(True)
    xd = [x.float().to(DEV).requires_grad_(True) for x in xs]
    rd = r.float().to(DEV).requires_grad_(True) if r is not None else None
    with T.step_guard(fp16=fp16, device=DEV) as guard:
        yp = T.linear_act([T.to_panel(x) for x in xd], widths, Wd, bd, rows, act, residual=None if rd is None else T.to_panel(rd))
        out = T.from_panel(yp, rows, N)
        out.backward((dy * 2.0 ** e).float().to(DEV))
        flagged = guard.overflowed()
    got = dict(y=out.detach().cpu(), dW=Wd.grad.cpu(), db=bd.grad.cpu())
    got.update({f"dx{i}": x.grad.cpu() for i, x in enumerate(xd)})
    if rd is not None:
        got["dres"] = rd.grad.cpu()
    return got, flagged


@pytest.mark.parametrize("e", U.LINEAR_GATED_EXPONENTS)
@pytest.mark.parametrize("case", list(U.LINEAR_CASES))
def test_linear_backward_holds_its_gate_down_to_2_to_the_minus_17(case, e):
    got, flagged = _linear(case, e)
    errs = U.linear_errors(case, e, got)
    _report(f"linear {case} e {e} fp16 True", errs)
    assert not flagged
    assert max(errs.values()) < U.GATE, errs


@pytest.mark.parametrize("e", U.LINEAR_REPORTED_EXPONENTS)
@pytest.mark.parametrize("case", list(U.LINEAR_CASES))
def test_linear_backward_below_2_to_the_minus_17_is_finite_and_unflagged(case, e):
    """Reported, not gated: the weight-gradient and data-gradient GEMMs still split du at the fixed scale, which is expected to exceed the
    gate here (DESIGN.md records the printed figures as an open item)."""
    got, flagged = _linear(case, e)
    errs = U.linear_errors(case, e, got)
    _report(f"linear {case} e {e} fp16 True (reported)", errs)
    assert not flagged
    assert all(x != float("inf") for x in errs.values()), errs       # linear_errors gives inf for a non-finite gradient
