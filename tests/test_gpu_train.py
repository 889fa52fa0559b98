"""Training primitives (first slice: the residual MLP of models/nets.py:19-30): HIP forward AND backward
through the C ABI (fc_train_*), against fp64 autograd of the pinned oracle's `mlp` / plain fp64 torch on the host."""
import pytest
import torch
import torch.nn.functional as F

import flowcompare_amd as fa
from flowcompare_amd import modules as M
from flowcompare_amd import train_ops as T
from knob_util import knobs
from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b, floor=1e-2):
    """max |a - b| relative to max |b| (floored: an identically-zero gradient, e.g. q of a one-key softmax, is compared absolutely)."""
    return (a.double().cpu() - b).abs().max().item() / max(floor, b.abs().max().item())


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("rows,widths,N,act,res", [(300, [150, 512], 512, "GELU", True), (1000, [150], 256, "RELU", False),
                                                   (257, [70, 33, 1], 300, None, False), (4096, [512], 3750, "ELU", False)])
def test_linear_act_forward_and_backward_match_fp64(rows, widths, N, act, res, fp16):
    g = torch.Generator().manual_seed(rows + N)
    K = sum(widths)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).double().requires_grad_(True)
    b = (torch.randn(N, generator=g) * 0.3).double().requires_grad_(True)
    xs = [torch.randn(rows, w, generator=g).double().requires_grad_(True) for w in widths]
    r = torch.randn(rows, N, generator=g).double().requires_grad_(True) if res else None
    dy = torch.randn(rows, N, generator=g).double()
    u = F.linear(torch.cat(xs, -1), W, b) + (r if res else 0)
    y = {"GELU": F.gelu, "RELU": F.relu, "ELU": F.elu, None: lambda t: t}[act](u)
    y.backward(dy)

    Wd, bd = W.detach().float().to(DEV).requires_grad_(True), b.detach().float().to(DEV).requires_grad_(True)
    xd = [x.detach().float().to(DEV).requires_grad_(True) for x in xs]
    rd = r.detach().float().to(DEV).requires_grad_(True) if res else None
    with T.step_guard(fp16=fp16, device=DEV) as guard:
        yp = T.linear_act([T.to_panel(x) for x in xd], widths, Wd, bd, rows, act, residual=None if rd is None else T.to_panel(rd))
        out = T.from_panel(yp, rows, N)
        out.backward(dy.float().to(DEV))
        assert not guard.overflowed()
    errs = dict(y=_rel(out.detach(), y.detach()), dW=_rel(Wd.grad, W.grad), db=_rel(bd.grad, b.grad))
    for i, (a, c) in enumerate(zip(xd, xs)):
        errs[f"dx{i}"] = _rel(a.grad, c.grad)
    if res:
        errs["dres"] = _rel(rd.grad, r.grad)
    print(f"rows {rows} widths {widths} N {N} act {act} fp16 {fp16}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < 5e-6, errs
    assert yp[:, N:].abs().sum().item() == 0.0                              # pad columns stay zero (zero weights and bias, act(0) = 0)


@pytest.mark.parametrize("config", ["frozen_weight", "no_bias", "second_input_only"])
def test_linear_act_computes_only_the_requested_gradients(config):
    """linear_act on 300 rows (one full 256-row tile and a partial one), segments [40, 33], N = 72, GELU, under step_guard, when only some
    gradients are asked for: weight frozen and bias trainable (the bias-only column-sum branch of the weight-gradient entry); bias=None
    (dW without db); only the second input requires grad (no weight-gradient call, one panel cut out of the data gradient).  Every
    requested gradient against fp64 autograd at the gate of test_linear_act_forward_and_backward_match_fp64, every other one None."""
    rows, widths, N = 300, [40, 33], 72
    K = sum(widths)
    g = torch.Generator().manual_seed(31)
    host = dict(W=torch.randn(N, K, generator=g) / K ** 0.5, b=torch.randn(N, generator=g) * 0.3,
                x0=torch.randn(rows, widths[0], generator=g), x1=torch.randn(rows, widths[1], generator=g))
    dy = torch.randn(rows, N, generator=g)
    if config == "no_bias":
        del host["b"]
    wanted = dict(W=config == "no_bias", b=config == "frozen_weight", x0=config != "second_input_only", x1=True)
    ref = {k: t.double().requires_grad_(True) for k, t in host.items()}
    yo = F.gelu(F.linear(torch.cat((ref["x0"], ref["x1"]), -1), ref["W"], ref.get("b")))
    yo.backward(dy.double())

    dev = {k: t.to(DEV).requires_grad_(wanted[k]) for k, t in host.items()}
    with T.step_guard(device=DEV) as guard:
        yp = T.linear_act([T.to_panel(dev["x0"]), T.to_panel(dev["x1"])], widths, dev["W"], dev.get("b"), rows, "GELU")
        out = T.from_panel(yp, rows, N)
        out.backward(dy.to(DEV))
        assert not guard.overflowed()
    errs = dict(y=_rel(out.detach(), yo.detach()))
    for k, t in dev.items():
        if wanted[k]:
            errs["d" + k] = _rel(t.grad, ref[k].grad)
        else:
            assert t.grad is None, k
    print(f"linear_act {config}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < 5e-6, errs


def test_weight_gradient_is_bit_reproducible_and_ignores_pad_rows():
    g = torch.Generator().manual_seed(5)
    rows, K, N = 1000, 150, 256
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV).requires_grad_(True)
    b = torch.zeros(N, device=DEV, requires_grad=True)
    x = T.to_panel(torch.randn(rows, K, generator=g).to(DEV))
    grads = []
    for junk in (0.0, 7.0):
        dy = torch.randn(x.shape[0], N, generator=torch.Generator().manual_seed(6)).to(DEV)
        dy[rows:] = dy[rows:] * junk + junk                            # rows beyond `rows` must never reach dW / db
        W.grad = b.grad = None
        y = T.linear_act([x], [K], W, b, rows, None)
        y.backward(dy)
        grads.append((W.grad.clone(), b.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


@pytest.mark.parametrize("act", ["GELU", "RELU"])
def test_mlp_at_coupling_widths_matches_oracle_autograd(act):
    """The coupling network of a C2 layer (cat(x1 150, attention 512) -> 512^3 -> 300, models/affine_coupling.py:33) on two panels:
    outputs and gradients of every parameter and both inputs against fp64 autograd through the pinned oracle's mlp()."""
    torch.manual_seed(3)
    mlp = M.MLP(662, [512, 512, 512], 300).to(DEV)
    rows = 700
    g = torch.Generator().manual_seed(4)
    x1, c = torch.randn(rows, 150, generator=g), torch.randn(rows, 512, generator=g)
    dy = torch.randn(rows, 300, generator=g)
    sd = {("m." + k): v.detach().cpu().double().requires_grad_(True) for k, v in mlp.state_dict().items()}
    x1o, co = x1.double().requires_grad_(True), c.double().requires_grad_(True)
    yo = O.mlp(sd, "m", torch.cat((x1o, co), -1), O._act(act))
    yo.backward(dy.double())

    x1d, cd = x1.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True)
    with T.step_guard(device=DEV) as guard:
        yp = T.mlp_panels(mlp, [T.to_panel(x1d), T.to_panel(cd)], [150, 512], rows, act)
        y = T.from_panel(yp, rows, 300)
        y.backward(dy.to(DEV))
        assert not guard.overflowed()
    errs = dict(y=_rel(y.detach(), yo.detach()), dx1=_rel(x1d.grad, x1o.grad), dc=_rel(cd.grad, co.grad))
    for k, p in mlp.named_parameters():
        errs["d" + k] = _rel(p.grad, sd["m." + k].grad)
    print(f"MLP 150|512 -> 512^3 -> 300, {act}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < 2e-5, errs


def test_fused_mlp_node_agrees_with_the_chain_of_linear_nodes(monkeypatch):
    """MlpFn (one autograd node; activation in the forward GEMM's epilogue, act' and the residual branch's gradient in the data-gradient
    GEMM's) against the same MLP as a chain of LinearActFn nodes with separate activation passes: same forward bits, gradients to
    fp32 rounding (the fused data gradient adds the residual branch before the products instead of after them).  Four hidden layers:
    keep / residual / keep / residual, so both kinds of hidden layer occur with and without a following residual."""
    torch.manual_seed(5)
    mlp = M.MLP(182, [512, 512, 512, 512, 512], 96).to(DEV)
    rows = 900
    g = torch.Generator().manual_seed(6)
    x1, c = torch.randn(rows, 150, generator=g).to(DEV), torch.randn(rows, 32, generator=g).to(DEV)
    dy = torch.randn(rows, 96, generator=g).to(DEV)
    out = {}
    for fused in (True, False):
        monkeypatch.setattr(T, "FUSED_MLP", fused)
        monkeypatch.setattr(T, "FUSED_ACT", fused)
        mlp.zero_grad()
        a, b = x1.clone().requires_grad_(True), c.clone().requires_grad_(True)
        with T.step_guard(device=DEV) as guard:
            y = T.from_panel(T.mlp_panels(mlp, [T.to_panel(a), T.to_panel(b)], [150, 32], rows, "GELU"), rows, 96)
            y.backward(dy)
            assert not guard.overflowed()
        out[fused] = (y.detach().clone(), a.grad.clone(), b.grad.clone(), [p.grad.clone() for p in mlp.parameters()])
    assert torch.equal(out[True][0], out[False][0])
    worst = max(_rel(out[True][1], out[False][1].double().cpu()), _rel(out[True][2], out[False][2].double().cpu()),
                max(_rel(p, q.double().cpu()) for p, q in zip(out[True][3], out[False][3])))
    print(f"fused MLP node vs chain of nodes: worst relative gradient difference {worst:.1e}")
    assert worst < 2e-6


def test_input_panel_wider_than_its_segment_gets_a_padded_gradient(monkeypatch):
    """Segments [40, 32] where the first input panel is 96 columns wide (its segment reads 64) and columns 40..95 hold random data, 300
    rows (one 256-row tile and a partial one): once through linear_act (N = 64) and once through the fused MlpFn node of
    MLP(72, [64, 64, 64], 32).  Outputs and every gradient against fp64 autograd on the true 40 + 32 columns (gates of
    test_linear_act_forward_and_backward_match_fp64 and test_mlp_at_coupling_widths_matches_oracle_autograd); the first input's gradient
    has the panel's shape and is exactly zero in the columns 64..95 that the segment does not read."""
    monkeypatch.setattr(T, "FUSED_MLP", True)
    monkeypatch.setattr(T, "FUSED_ACT", True)
    rows, widths, wide = 300, [40, 32], 96
    g = torch.Generator().manual_seed(17)
    x0, x1 = torch.randn(rows, 40, generator=g), torch.randn(rows, 32, generator=g)
    junk = torch.randn(rows, wide - 40, generator=g)
    W = torch.randn(64, 72, generator=g) / 72 ** 0.5
    b = torch.randn(64, generator=g) * 0.3
    torch.manual_seed(18)
    mlp = M.MLP(72, [64, 64, 64], 32).to(DEV)

    def panels():
        p0 = torch.zeros(T._round_up(rows, T.ROW_PAD), wide)
        p0[:rows, :40], p0[:rows, 40:] = x0, junk
        return p0.to(DEV).requires_grad_(True), T.to_panel(x1.to(DEV)).requires_grad_(True)

    def check_inputs(errs, p0, p1, x0o, x1o):
        assert p0.grad.shape == p0.shape and p0.grad[:, 64:].abs().max().item() == 0.0
        errs["dx0"], errs["dx1"] = _rel(p0.grad[:rows, :40], x0o.grad), _rel(p1.grad[:rows, :32], x1o.grad)

    # ---- one Linear
    dy = torch.randn(rows, 64, generator=g)
    Wo, bo = W.double().requires_grad_(True), b.double().requires_grad_(True)
    x0o, x1o = x0.double().requires_grad_(True), x1.double().requires_grad_(True)
    yo = F.gelu(F.linear(torch.cat((x0o, x1o), -1), Wo, bo))
    yo.backward(dy.double())
    Wd, bd = W.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    p0, p1 = panels()
    with T.step_guard(device=DEV) as guard:
        y = T.from_panel(T.linear_act([p0, p1], widths, Wd, bd, rows, "GELU"), rows, 64)
        y.backward(dy.to(DEV))
        assert not guard.overflowed()
    errs = dict(y=_rel(y.detach(), yo.detach()), dW=_rel(Wd.grad, Wo.grad), db=_rel(bd.grad, bo.grad))
    check_inputs(errs, p0, p1, x0o, x1o)
    print("linear_act, panel 96 wide for a 40-column segment: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < 5e-6, errs

    # ---- the fused MLP node
    dy = torch.randn(rows, 32, generator=g)
    sd = {("m." + k): v.detach().cpu().double().requires_grad_(True) for k, v in mlp.state_dict().items()}
    x0o, x1o = x0.double().requires_grad_(True), x1.double().requires_grad_(True)
    yo = O.mlp(sd, "m", torch.cat((x0o, x1o), -1), O._act("GELU"))
    yo.backward(dy.double())
    p0, p1 = panels()
    with T.step_guard(device=DEV) as guard:
        yp = T.mlp_panels(mlp, [p0, p1], widths, rows, "GELU")
        assert type(yp.grad_fn).__name__.startswith("MlpFn")
        y = T.from_panel(yp, rows, 32)
        y.backward(dy.to(DEV))
        assert not guard.overflowed()
    errs = dict(y=_rel(y.detach(), yo.detach()))
    check_inputs(errs, p0, p1, x0o, x1o)
    for k, p in mlp.named_parameters():
        errs["d" + k] = _rel(p.grad, sd["m." + k].grad)
    print("MLP 72 -> 64^3 -> 32 (fused node), panel 96 wide for a 40-column segment: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < 2e-5, errs


def test_mlp_forward_on_plain_tensors_and_range_guard():
    torch.manual_seed(8)
    mlp = M.MLP(6, [64, 64, 64], 32).to(DEV)
    x = torch.randn(2, 50, 6, device=DEV, requires_grad=True)
    with T.step_guard(device=DEV) as guard:
        y = T.mlp_forward(mlp, x, "GELU")
        y.sum().backward()
        assert not guard.overflowed()
    sd = {("m." + k): v.detach().cpu().double() for k, v in mlp.state_dict().items()}
    assert y.shape == (2, 50, 32) and _rel(y.detach(), O.mlp(sd, "m", x.detach().cpu().double(), F.gelu)) < 5e-6
    ref = mlp.in_layer.weight.grad.clone()
    # outside the fp16 range the flag comes back set; the fp32-input loop then gives the answer
    big = (x.detach() * 1e5).requires_grad_(True)
    with T.step_guard(device=DEV) as guard:
        T.mlp_forward(mlp, big, "RELU").sum().backward()
        assert guard.overflowed()
    mlp.zero_grad()
    with T.step_guard(fp16=False, device=DEV) as guard:
        y32 = T.mlp_forward(mlp, big, "RELU")
        y32.sum().backward()
        assert not guard.overflowed()
    want = O.mlp(sd, "m", big.detach().cpu().double(), F.relu)
    assert _rel(y32.detach(), want) < 5e-6
    assert torch.isfinite(mlp.in_layer.weight.grad).all() and ref.shape == mlp.in_layer.weight.grad.shape


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("B,N,M,I", [(2, 300, 77, 64), (3, 130, 1000, 64), (2, 50, 40, 8), (1, 1, 1, 64)])
def test_attention_forward_and_backward_match_fp64(B, N, M, I, fp16):
    g = torch.Generator().manual_seed(B * N + M)
    q = torch.randn(B, N, I, generator=g).double().requires_grad_(True)
    k = torch.randn(B, M, I, generator=g).double().requires_grad_(True)
    v = torch.randn(B, M, I, generator=g).double().requires_grad_(True)
    dout = torch.randn(B, N, I, generator=g).double()
    scale = I ** -0.5
    out = torch.softmax(q @ k.transpose(1, 2) * scale, -1) @ v
    out.backward(dout)
    qd, kd, vd = (t.detach().float().to(DEV).requires_grad_(True) for t in (q, k, v))
    with T.step_guard(fp16=fp16, device=DEV) as guard:
        op = T.attention(T.to_panel(qd.reshape(B * N, I)), T.to_panel(kd.reshape(B * M, I)), T.to_panel(vd.reshape(B * M, I)), B, N, M, scale)
        o = T.from_panel(op, B * N, I).reshape(B, N, I)
        o.backward(dout.float().to(DEV))
        assert not guard.overflowed()
    # dS = P (dP - dO.O): the difference of two O(|dO| |v| sqrt(I)) sums, so its fp32 error is absolute at that scale (floor 1)
    errs = dict(out=_rel(o.detach(), out.detach()), dq=_rel(qd.grad, q.grad, 1.0), dk=_rel(kd.grad, k.grad, 1.0), dv=_rel(vd.grad, v.grad))
    print(f"attention B {B} N {N} M {M} I {I} fp16 {fp16}: " + " ".join(f"{a} {b:.1e}" for a, b in errs.items()))
    assert max(errs.values()) < 5e-6, errs


@pytest.mark.parametrize("spread", [0.5, 1.5])
@pytest.mark.parametrize("K,d2,rows", [(8, 150, 300), (4, 6, 70), (16, 33, 257)])
def test_spline_forward_and_backward_match_oracle_autograd(K, d2, rows, spread):
    """The training spline element against fp64 autograd through the pinned oracle's rq_spline (reference layout [d2][3K+1]);
    inputs cover the tails (|x| > 3: identity, zero parameter gradient), every bin and the +bound knot.  With widely spread logits
    (1.5) some bins are ~0.01 wide with slopes of several hundred, where fp32 itself is ill-conditioned (knot rounding times slope):
    there the gate is the error of the SAME oracle run in fp32 (eager PyTorch, i.e. what the reference's own training computes)."""
    g = torch.Generator().manual_seed(K + d2)
    x = (torch.rand(rows, d2, generator=g) * 8 - 4).double()
    x[0, :3] = torch.tensor([-3.0, 3.0, 0.0], dtype=torch.float64)
    p = (torch.randn(rows, d2, 3 * K + 1, generator=g) * spread).double()
    gy, gl = torch.randn(rows, d2, generator=g).double(), torch.randn(rows, generator=g).double()

    def oracle(dtype):
        xx, pp = x.detach().clone().to(dtype).requires_grad_(True), p.detach().clone().to(dtype).requires_grad_(True)
        y, lad = O.rq_spline(xx, pp[..., :K], pp[..., K:2 * K], pp[..., 2 * K:])
        ((y * gy.to(dtype)).sum() + (lad.sum(-1) * gl.to(dtype)).sum()).backward()
        return y.detach().double(), lad.sum(-1).detach().double(), xx.grad.double(), pp.grad.double()
    y, ldj64, dx, dp = oracle(torch.float64)
    y32, ldj32, dx32, dp32 = oracle(torch.float32)
    xd = x.float().to(DEV).requires_grad_(True)
    pd = p.float().to(DEV).requires_grad_(True)
    yp, ldj = T.rq_spline(T.to_panel(xd), T.to_panel(pd.reshape(rows, -1)), rows, d2, K)
    yy, ll = T.from_panel(yp, rows, d2), ldj[:rows]
    ((yy * gy.float().to(DEV)).sum() + (ll * gl.float().to(DEV)).sum()).backward()
    errs = dict(y=_rel(yy.detach(), y), ldj=_rel(ll.detach(), ldj64), dx=_rel(xd.grad, dx), dp=_rel(pd.grad, dp))
    ref32 = dict(y=_rel(y32, y), ldj=_rel(ldj32, ldj64), dx=_rel(dx32, dx), dp=_rel(dp32, dp))
    print(f"spline K {K} d2 {d2} rows {rows} spread {spread}: " + " ".join(f"{a} {b:.1e} (fp32 oracle {ref32[a]:.1e})" for a, b in errs.items()))
    for name in errs:
        assert errs[name] < 3.0 * ref32[name] + 5e-6, (name, errs[name], ref32[name])
    assert yp[:, d2:].abs().sum().item() == 0.0


@pytest.mark.parametrize("rows,grad_scale", [(700, 1.0), (1000, 1e-5), (300, 300.0)])
def test_spline_parameter_layer_on_the_wide_loop_matches_fp64_and_the_fp32a_loop(rows, grad_scale):
    """Round 4: in a training step the spline parameter layer (512 -> 3750, models/spline_coupling.py:187-210 behind models/nets.py:19-30) runs its
    forward and its data gradient on the 256 x 256 one-accumulator loop (csrc/spline_wide.hip EPI 3; csrc/train_linear.hip routes layers with at
    least 1024 outputs): activations are split into limbs after their LDS read at a constant scale, the gradient panel at one exact
    power-of-two scale PER ROW taken from the row maxima the spline backward writes beside it.  Coupling net + spline + backward against
    fp64 autograd through the pinned oracle, no worse than the fp32-A loop (debug knob 31 = 0) -- at gradient magnitudes of a loss that is
    a mean over 65 536 points (1e-5), of order one, and large (300)."""
    K, d1, d2 = 8, 150, 150
    torch.manual_seed(11)
    mlp = M.MLP(d1 + 64, [512, 512], d2 * (3 * K + 1)).to(DEV)
    with torch.no_grad():
        mlp.out_layer.weight.mul_(0.5)
    g = torch.Generator().manual_seed(rows)
    x1, c = torch.randn(rows, d1, generator=g), torch.randn(rows, 64, generator=g)
    x2 = torch.rand(rows, d2, generator=g) * 7 - 3.5
    gy, gl = torch.randn(rows, d2, generator=g) * grad_scale, torch.randn(rows, generator=g) * grad_scale

    sd = {("m." + k): v.detach().cpu().double().requires_grad_(True) for k, v in mlp.state_dict().items()}
    x1o, co, x2o = x1.double().requires_grad_(True), c.double().requires_grad_(True), x2.double().requires_grad_(True)
    po = O.mlp(sd, "m", torch.cat((x1o, co), -1), O._act("GELU")).reshape(rows, d2, 3 * K + 1)
    yo, lado = O.rq_spline(x2o, po[..., :K], po[..., K:2 * K], po[..., 2 * K:])
    ((yo * gy.double()).sum() + (lado.sum(-1) * gl.double()).sum()).backward()

    def run(wide):
        mlp.zero_grad()
        a, b, xx = x1.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True), x2.to(DEV).requires_grad_(True)
        with T.step_guard(device=DEV) as guard:
            pp = T.mlp_panels(mlp, [T.to_panel(a), T.to_panel(b)], [d1, 64], rows, "GELU")
            yp, ldj = T.rq_spline(T.to_panel(xx), pp, rows, d2, K)
            ((T.from_panel(yp, rows, d2) * gy.to(DEV)).sum() + (ldj[:rows] * gl.to(DEV)).sum()).backward()
            assert not guard.overflowed()
        errs = dict(y=_rel(T.from_panel(yp, rows, d2).detach(), yo.detach()), ldj=_rel(ldj[:rows].detach(), lado.sum(-1).detach()),
                    dx1=_rel(a.grad, x1o.grad, floor=1e-2 * grad_scale), dc=_rel(b.grad, co.grad, floor=1e-2 * grad_scale),
                    dx2=_rel(xx.grad, x2o.grad, floor=1e-2 * grad_scale))
        for k, q in mlp.named_parameters():
            errs["d" + k] = _rel(q.grad, sd["m." + k].grad, floor=1e-2 * grad_scale)
        return errs
    with knobs({31: 1}):
        wide = run(True)
    with knobs({31: 0}):
        base = run(False)
    print(f"rows {rows} gradient scale {grad_scale}: wide loop " + " ".join(f"{k} {v:.1e}" for k, v in wide.items()))
    print(f"{'':>{len(str(rows)) + len(str(grad_scale)) + 22}}fp32-A loop " + " ".join(f"{k} {v:.1e}" for k, v in base.items()))
    for k in wide:
        assert wide[k] < 2.0 * base[k] + 2e-6, (k, wide[k], base[k])


def _spline_layer_step(hook=None, wide=True):
    """One forward + backward of the coupling net MLP(214, [512, 512], 3750) + spline (K 8, d1 = d2 = 150, 300 rows, rows_pad 512, gradients
    of order one) under step_guard with the in-library profile on; `hook` is registered on the MLP's output panel.  Returns (launches of
    the 256 x 256 one-accumulator kernel, range flag, [a.grad, b.grad, xx.grad, every MLP parameter's gradient])."""
    from flowcompare_amd import engine
    K, d1, d2, rows = 8, 150, 150, 300
    torch.manual_seed(11)
    mlp = M.MLP(d1 + 64, [512, 512], d2 * (3 * K + 1)).to(DEV)
    with torch.no_grad():
        mlp.out_layer.weight.mul_(0.5)
    g = torch.Generator().manual_seed(rows)
    x1, c = torch.randn(rows, d1, generator=g), torch.randn(rows, 64, generator=g)
    x2 = torch.rand(rows, d2, generator=g) * 7 - 3.5
    gy, gl = torch.randn(rows, d2, generator=g), torch.randn(rows, generator=g)
    a, b, xx = x1.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True), x2.to(DEV).requires_grad_(True)
    try:
        engine.profile_enable(True); engine.profile_stride(1); engine.profile_reset()
        with knobs({31: 1 if wide else 0}), T.step_guard(device=DEV) as guard:
            pp = T.mlp_panels(mlp, [T.to_panel(a), T.to_panel(b)], [d1, 64], rows, "GELU")
            if hook is not None:
                pp.register_hook(hook)
            yp, ldj = T.rq_spline(T.to_panel(xx), pp, rows, d2, K)
            ((T.from_panel(yp, rows, d2) * gy.to(DEV)).sum() + (ldj[:rows] * gl.to(DEV)).sum()).backward()
            overflowed = guard.overflowed()
        launches = sum(r["launches"] for r in engine.profile_report() if r["kernel"].startswith("void fc::spline_wide_kernel<3,"))
    finally:
        engine.profile_enable(False); engine.profile_stride(1); engine.profile_reset()
    return launches, overflowed, [a.grad, b.grad, xx.grad] + [q.grad for q in mlp.parameters()]


def test_spline_row_maxima_reach_the_parameter_layers_data_gradient():
    """The handoff is visible: SplineFn.backward records the row maxima on the gradient panel it returns, MlpFn.backward finds them on
    its incoming panel and the out layer's data gradient runs on the one-accumulator loop -- 2 launches of that kernel per step (the out
    layer's forward and its data gradient), none with knob 31 = 0."""
    launches, overflowed, _ = _spline_layer_step()
    launches0, overflowed0, _ = _spline_layer_step(wide=False)
    print(f"one-accumulator launches per step: {launches} (knob 31 = 0: {launches0}), range flag {overflowed} / {overflowed0}")
    assert launches == 2 and not overflowed
    assert launches0 == 0 and not overflowed0


def test_an_edited_gradient_panel_is_not_paired_with_stale_row_maxima():
    """A hook that scales the MLP output's gradient IN PLACE leaves the panel object -- and the record on it -- in place, but bumps its version
    counter: the lookup misses and the data gradient runs on the fp32-A loop (1 one-accumulator launch, the forward), on the same operands
    as with a hook that returns a new tensor (which never carried a record): every gradient bit for bit the same."""
    n_in, ovf_in, g_in = _spline_layer_step(hook=lambda g: g.mul_(1000.0))
    n_new, ovf_new, g_new = _spline_layer_step(hook=lambda g: g * 1000.0)
    print(f"one-accumulator launches per step: in-place hook {n_in}, new-tensor hook {n_new}; range flag {ovf_in} / {ovf_new}; "
          f"gradients equal: {[torch.equal(p, q) for p, q in zip(g_in, g_new)]}")
    assert n_in == 1 and not ovf_in
    assert n_new == 1 and not ovf_new
    assert len(g_in) == len(g_new) == 9
    for p, q in zip(g_in, g_new):
        assert torch.equal(p, q)


def test_spline_backward_writes_the_row_maxima_into_the_callers_buffer():
    """fc_train_rqspline_bwd_f32 with an explicit row_absmax buffer (K 8, d2 150, 300 rows, the inputs of the spline test above): entry r is
    max |dparams[r, :]| exactly (a maximum does not round), the tail up to rows_pad is zeroed, a row with a NaN (through dldj) reads +inf;
    with a NULL buffer dx2 and dparams come out bit for bit the same."""
    from flowcompare_amd import engine
    L = engine.lib()
    K, d2, rows = 8, 150, 300
    g = torch.Generator().manual_seed(K + d2)
    x = torch.rand(rows, d2, generator=g) * 8 - 4
    x[0, :3] = torch.tensor([-3.0, 3.0, 0.0])
    p = torch.randn(rows, d2, 3 * K + 1, generator=g) * 0.5
    gy, gl = torch.randn(rows, d2, generator=g), torch.randn(rows, generator=g)
    x2, params, dy2 = T.to_panel(x.to(DEV)), T.to_panel(p.reshape(rows, -1).to(DEV)), T.to_panel(gy.to(DEV))
    rows_pad = x2.shape[0]
    assert rows_pad == 512 and params.shape[1] % 64 == 0

    def bwd(dldj, with_buffer=True):
        dx2 = T._panel_out(rows_pad, x2.shape[1], rows, DEV)
        dparams = T._panel_out(rows_pad, params.shape[1], rows, DEV)
        rowmax = torch.full((rows_pad,), -1.0, device=DEV) if with_buffer else None
        L.fc_train_rqspline_bwd_f32(engine._ptr(x2), x2.shape[1], engine._ptr(params), params.shape[1], engine._ptr(dy2), dy2.shape[1], engine._ptr(dldj),
                                    engine._ptr(dx2), dx2.shape[1], engine._ptr(dparams), dparams.shape[1], rows, d2, K, engine._ptr(rowmax), engine._stream())
        torch.cuda.synchronize()
        return dx2, dparams, rowmax
    dldj = torch.zeros(rows_pad, device=DEV)
    dldj[:rows] = gl.to(DEV)
    dx2, dparams, rowmax = bwd(dldj)
    assert torch.equal(rowmax[:rows], dparams[:rows].abs().amax(1))
    assert rowmax[:rows].min().item() > 0.0
    assert torch.equal(rowmax[rows:], torch.zeros(rows_pad - rows, device=DEV))
    dx2_0, dparams_0, _ = bwd(dldj, with_buffer=False)
    assert torch.equal(dx2_0, dx2) and torch.equal(dparams_0, dparams)
    bad = dldj.clone()
    bad[7] = float("nan")
    _, dparams_n, rowmax_n = bwd(bad)
    assert torch.isnan(dparams_n[7]).any()
    assert rowmax_n[7].item() == float("inf")
    keep = torch.arange(rows, device=DEV) != 7
    assert torch.equal(rowmax_n[:rows][keep], rowmax[:rows][keep]) and torch.equal(rowmax_n[rows:], rowmax[rows:])


@pytest.mark.parametrize("rows,width", [(300, 256), (1000, 8), (5, 100)])
def test_layernorm_forward_and_backward_match_fp64(rows, width):
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, width, generator=g) * 2 + 0.5).double().requires_grad_(True)
    gamma = (torch.rand(width, generator=g) + 0.5).double().requires_grad_(True)
    beta = torch.randn(width, generator=g).double().requires_grad_(True)
    dy = torch.randn(rows, width, generator=g).double()
    y = F.layer_norm(x, (width,), gamma, beta, 1e-5)
    y.backward(dy)
    xd, gd, bd = (t.detach().float().to(DEV).requires_grad_(True) for t in (x, gamma, beta))
    yp = T.layer_norm(T.to_panel(xd), gd, bd, rows)
    yy = T.from_panel(yp, rows, width)
    yy.backward(dy.float().to(DEV))
    errs = dict(y=_rel(yy.detach(), y.detach()), dx=_rel(xd.grad, x.grad), dgamma=_rel(gd.grad, gamma.grad), dbeta=_rel(bd.grad, beta.grad))
    print(f"layernorm rows {rows} width {width}: " + " ".join(f"{a} {b:.1e}" for a, b in errs.items()))
    assert max(errs.values()) < 5e-6, errs


# ---------------------------------------------------------------- the whole flow: loss.backward() against the reference's gradients
import json
import os

import numpy as np

from conftest import GOLDEN, Fixture
from flowcompare_amd import train_flow as TF
import synth

HEAD = 8


def _build(fx):
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    sd_flow, sd_emb = fx.state_dicts()
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    return cfg, md


def _train_step(fx, cfg, md, fp16=True, **flow_kw):
    Din = cfg["input_dim"]
    e0, e1, ex = fx.t("extract_0").to(DEV), fx.t("extract_1").to(DEV), fx.t("extra")
    with torch.no_grad():
        ctx = md["input_embedder"](e0[:, :, :Din])
    if ctx.dim() == 2:                                               # global embedder: one vector per scene, repeated per target point
        ctx = ctx[:, None, :].expand(-1, e1.shape[1], -1).contiguous()
    ctx = ctx.detach().requires_grad_(True)
    x = e1[:, :, :Din].clone().requires_grad_(True)
    extra = None if ex is None else ex.to(DEV)[:, None, :].expand(-1, e1.shape[1], -1)
    md["flow"].zero_grad()
    with T.step_guard(fp16=fp16, device=DEV) as guard:
        lp = TF.flow_log_prob(md["flow"], x, ctx, extra, [e.to(DEV) for e in fx.eps()], **flow_kw)
        loss = -lp.mean()
        loss.backward()
        assert not guard.overflowed()
    return loss, lp, x, ctx


@pytest.mark.parametrize("case", ["tiny_spline_relu", "tiny_affine", "spline_L2", "tiny_cif", "tiny_global_extra", "tiny_random_permute", "paconv_L2"])
def test_flow_backward_matches_reference_gradients(case):
    """loss.backward() through the HIP training path against the gradients the REFERENCE produced for the same weights, inputs and
    noise (tests/golden/grad_*.npz, eval mode): every flow parameter through sum / L1 / random projection / first entries, and
    d loss / d extract_1."""
    fx = Fixture("e2e_" + case)
    z = np.load(os.path.join(GOLDEN, "grad_" + case + ".npz"))
    cfg, md = _build(fx)
    loss, lp, x, ctx = _train_step(fx, cfg, md)
    assert abs(loss.item() - float(z["eval/loss"])) < 2e-4 * max(1.0, abs(float(z["eval/loss"])))
    assert np.abs(lp.detach().cpu().double().numpy() - fx.a["log_prob_f64"]).max() < 2e-3
    gnorm = float(z["eval/grad_norm"])
    dx_err = np.abs(x.grad.cpu().double().numpy() - z["eval/d_extract_1"]).max() / max(1e-12, np.abs(z["eval/d_extract_1"]).max())
    names = [n for n in json.loads(bytes(z["names_json"]).decode())["eval"] if n.startswith("flow/")]
    params = {}
    for n, p_ in md["flow"].named_parameters():
        params[n] = p_
        params[n.replace(".augmenter.noise_dist.", ".slicer.noise_dist.")] = p_      # CIFblock: ONE ConditionalNormal under two names
    # the same step through the pinned oracle in fp32 (eager PyTorch = the arithmetic the reference itself trains in): its distance
    # from the fp64 reference gradients is the conditioning of the problem, and the yardstick for the HIP path
    c = fx.derived_cfg()
    sd32, _ = fx.state_dicts(torch.float32)
    for v in sd32.values():
        if v.is_floating_point():
            v.requires_grad_(True)
    ex = fx.t("extra", torch.float32)
    ex = None if ex is None else ex[:, None, :].expand(-1, fx.meta["N"], -1)
    lp32 = O.flow_log_prob(c, sd32, fx.t("extract_1", torch.float32)[:, :, :c["input_dim"]], ctx.detach().cpu(), ex, fx.eps(torch.float32))
    (-lp32.mean()).backward()

    def summary(g, key):
        g = g.double().cpu().reshape(-1)
        r = torch.from_numpy(synth.normal("gradproj/" + key, (g.numel(),), 0))
        return np.concatenate([[g.sum().item(), g.abs().sum().item(), (g * r).sum().item()], np.pad(g[:HEAD].numpy(), (0, max(0, HEAD - g.numel())))])
    worst, worst_name, worst32 = 0.0, "", 0.0
    for key in names:
        n = key.split("/", 1)[1]
        assert params[n].grad is not None, key
        want = z["eval/" + key]
        scale = max(want[1], 1e-6 * gnorm)
        err = np.abs(summary(params[n].grad, key) - want).max() / scale
        err32 = np.abs(summary(sd32[n.replace(".slicer.noise_dist.", ".augmenter.noise_dist.")].grad, key) - want).max() / scale
        worst32 = max(worst32, err32)
        assert err < 1e-3, (key, err, err32)
        if err > worst:
            worst, worst_name = err, key
    print(f"{case}: loss {loss.item():.6f} (ref {float(z['eval/loss']):.6f}); d extract_1 rel err {dx_err:.1e}; {len(names)} flow parameter "
          f"gradients, worst error / L1 norm {worst:.1e} ({worst_name}); fp32 oracle's worst {worst32:.1e}")
    # (+1e-4: tensors whose exact gradient is zero -- q-side weights under a context of identical keys, global embedder -- hold only
    #  rounding noise, measured against the 1e-6 |g| floor above)
    # paconv_L2 (affine layers at the real widths, 256 context points): the gradients of the pre-attention MLP weights -- which pass the
    # LayerNorm and the softmax -- sit at 3-7e-4 of their L1 norm on the split-fp16 AND on the fp32-input kernels alike
    # (profiles/micro/grad_noise_check.py), an order above eager fp32 PyTorch on this fixture; every other tensor is below 1e-4
    assert dx_err < 2e-4 and worst < (1e-3 if case == "paconv_L2" else 3.0 * worst32 + 1e-4)


def test_flow_backward_with_extra_context_matches_oracle_autograd():
    """C4 structure at the real widths (dulcet: affine sigmoid coupling, extra z-value context, 3 layers): parameter gradients and the
    gradient w.r.t. the CONTEXT EMBEDDING (what the embedder's backward will consume) against fp64 autograd through the pinned oracle."""
    fx = Fixture("e2e_dulcet_L3")
    cfg, md = _build(fx)
    loss, lp, x, ctx = _train_step(fx, cfg, md)
    c = fx.derived_cfg()
    sd_f, _ = fx.state_dicts(torch.float64)
    for v in sd_f.values():
        if v.is_floating_point():
            v.requires_grad_(True)
    e1 = fx.t("extract_1", torch.float64)[:, :, :c["input_dim"]].requires_grad_(True)
    ctx_o = ctx.detach().cpu().double().requires_grad_(True)
    ex = fx.t("extra", torch.float64)[:, None, :].expand(-1, e1.shape[1], -1)
    lp_o = O.flow_log_prob(c, sd_f, e1, ctx_o, ex, fx.eps(torch.float64))
    (-lp_o.mean()).backward()
    errs = dict(loss=abs(loss.item() + lp_o.mean().item()), dx=_rel(x.grad, e1.grad), dctx=_rel(ctx.grad, ctx_o.grad))
    worst, worst_name = 0.0, ""
    for n, p in md["flow"].named_parameters():
        if sd_f[n].grad is None:
            continue
        e = (p.grad.double().cpu() - sd_f[n].grad).abs().sum().item() / max(sd_f[n].grad.abs().sum().item(), 1e-9)
        if e > worst:
            worst, worst_name = e, n
    print(f"dulcet_L3: loss diff {errs['loss']:.1e} dx {errs['dx']:.1e} dctx {errs['dctx']:.1e}; worst parameter gradient L1 error {worst:.1e} ({worst_name})")
    assert errs["loss"] < 2e-4 and errs["dx"] < 2e-4 and errs["dctx"] < 2e-4 and worst < 2e-4


def test_deep_stack_gradients_are_as_close_to_fp64_as_eager_fp32(monkeypatch):
    """Module-initialised weights make a deep stack ill-conditioned (the forward already differs by O(1e-3) nats between fp32 and fp64
    at 8 layers, tests/test_gpu_fullsize.py): the whole-gradient distance of the HIP training path from fp64 autograd through the
    pinned oracle must be no worse than that of the same oracle in fp32 (eager PyTorch, the arithmetic the reference trains in)."""
    cfg = fa.named_config("c2_dgcnn_attn_spline", n_flow_layers=8, sample_size=192)
    torch.manual_seed(21)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    for m in md["flow"].modules():
        if hasattr(m, "initialized"):
            m.initialized.fill_(1.0)
    g = torch.Generator().manual_seed(22)
    B, N, Mc = 2, 192, 200
    x = torch.rand(B, N, 6, generator=g)
    ctx = torch.randn(B, Mc, 64, generator=g) * 0.5
    eps = [torch.randn(B, N, 294, generator=g)]
    md["flow"].zero_grad()
    # the magnitude of the upstream gradient that a real step hands the operators (printed only: test_gpu_train_grad_scale.py relates its
    # exponents to these): max |dout| per call of the attention backward and of the Linear backward, in the order autograd runs them
    seen = {"attention": [], "linear": []}

    def recorded(fn, key):
        def backward(ctx_, dy, *rest):
            seen[key].append(dy.detach().abs().max().item())
            return fn(ctx_, dy, *rest)
        return staticmethod(backward)
    monkeypatch.setattr(T.AttentionFn, "backward", recorded(T.AttentionFn.backward, "attention"))
    monkeypatch.setattr(T.LinearActFn, "backward", recorded(T.LinearActFn.backward, "linear"))
    with T.step_guard(device=DEV) as guard:
        lp = TF.flow_log_prob(md["flow"], x.to(DEV), ctx.to(DEV), None, [e.to(DEV) for e in eps])
        (-lp.mean()).backward()
        assert not guard.overflowed()
    for key, vals in seen.items():
        if vals:
            print(f"8 layers at real widths: max |dout| at the {key} backward: first call {vals[0]:.2e}, {len(vals)} calls, "
                  f"smallest {min(vals):.2e}, largest {max(vals):.2e}")
    c = dict(cfg)

    def oracle(dtype):
        sd = {k: v.detach().cpu().to(dtype) if v.is_floating_point() else v.cpu() for k, v in md["flow"].state_dict().items()}
        for v in sd.values():
            if v.is_floating_point():
                v.requires_grad_(True)
        lo = O.flow_log_prob(c, sd, x.to(dtype), ctx.to(dtype), None, [e.to(dtype) for e in eps])
        (-lo.mean()).backward()
        return lo.detach().double(), sd
    lp64, sd64 = oracle(torch.float64)
    lp32, sd32 = oracle(torch.float32)
    num_h = num_32 = den = 0.0
    for n, p in md["flow"].named_parameters():
        if sd64[n].grad is None:
            continue
        g64 = sd64[n].grad
        num_h += float(((p.grad.double().cpu() - g64) ** 2).sum())
        num_32 += float(((sd32[n].grad.double() - g64) ** 2).sum())
        den += float((g64 ** 2).sum())
    e_h, e_32 = (num_h / den) ** 0.5, (num_32 / den) ** 0.5
    d_h, d_32 = (lp.detach().cpu().double() - lp64).abs().max().item(), (lp32 - lp64).abs().max().item()
    print(f"8 layers at real widths: |g - g64| / |g64|: HIP {e_h:.2e}, fp32 oracle {e_32:.2e}; log-prob max diff: HIP {d_h:.2e}, fp32 oracle {d_32:.2e}")
    assert e_h < 3.0 * e_32 + 1e-5


@pytest.mark.parametrize("case", ["tiny_affine", "tiny_spline_relu", "tiny_cif", "spline_L2"])
def test_actnorm_data_dependent_init_matches_reference(case):
    """First training forward with every ActNorm un-initialised (act_norm.py:27-39): the statistics each layer takes from its input and
    the resulting log-probs against the reference's own first batch (tests/golden/grad_*.npz, record "init")."""
    fx = Fixture("e2e_" + case)
    z = np.load(os.path.join(GOLDEN, "grad_" + case + ".npz"))
    cfg, md = _build(fx)
    md["flow"].train()
    old = {}
    for n, m in md["flow"].named_modules():
        if hasattr(m, "initialized"):
            m.initialized.zero_()
            old[n] = m.shift
    loss, lp, x, ctx = _train_step(fx, cfg, md)
    assert np.abs(lp.detach().cpu().double().numpy() - z["init/log_prob"]).max() < 2e-3
    worst = 0.0
    for n, m in md["flow"].named_modules():
        if hasattr(m, "initialized"):
            assert float(m.initialized) == 1.0 and m.shift is not old[n]          # replaced Parameter objects, like the reference
            for leaf in ("shift", "log_scale"):
                want = z[f"init/{n}.{leaf}"]
                worst = max(worst, np.abs(getattr(m, leaf).detach().cpu().double().numpy() - want).max() / max(1.0, np.abs(want).max()))
    print(f"{case}: ActNorm data-dependent init, worst statistic error {worst:.1e}; loss {loss.item():.5f} (ref {float(z['init/loss']):.5f})")
    assert worst < 1e-4
    md["flow"].eval()


@pytest.mark.parametrize("case", ["tiny_affine", "tiny_spline_relu", "spline_L2", "tiny_global_extra", "paconv_L2"])
def test_full_training_step_matches_reference_train_mode_gradients(case):
    """The WHOLE path in train() mode -- DGCNN embedder with BatchNorm batch statistics, flow, loss.backward() -- against the gradients
    the reference produced in train mode for the same weights, inputs and noise (tests/golden/grad_*.npz, record "train"): every
    embedder and flow parameter, d loss / d extract_1, and the BatchNorm running statistics torch would have after the step."""
    from flowcompare_amd import train_embed
    fx = Fixture("e2e_" + case)
    z = np.load(os.path.join(GOLDEN, "grad_" + case + ".npz"))
    cfg, md = _build(fx)
    md["flow"].train()
    md["input_embedder"].train()
    Din = cfg["input_dim"]
    e0, e1, ex = fx.t("extract_0").to(DEV), fx.t("extract_1").to(DEV), fx.t("extra")
    bn1 = next(m for m in md["input_embedder"].modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm))     # DGCNN: bn1; PAConv: the first ScoreNet's
    bn1_mean_before = bn1.running_mean.clone()
    x = e1[:, :, :Din].clone().requires_grad_(True)
    for m in (md["flow"], md["input_embedder"]):
        m.zero_grad()
    with T.step_guard(device=DEV) as guard:
        loss, lp, _ = fa.inner_loop((e0, x, None if ex is None else ex.to(DEV)), md, cfg, eps=[e.to(DEV) for e in fx.eps()])
        loss.backward()
        assert not guard.overflowed()
    assert abs(loss.item() - float(z["train/loss"])) < 2e-4 * max(1.0, abs(float(z["train/loss"])))
    gnorm = float(z["train/grad_norm"])
    dx_err = np.abs(x.grad.cpu().double().numpy() - z["train/d_extract_1"]).max() / max(1e-12, np.abs(z["train/d_extract_1"]).max())
    names = json.loads(bytes(z["names_json"]).decode())["train"]
    params = {}
    for part in ("flow", "input_embedder"):
        for n, p_ in md[part].named_parameters():
            params[f"{part}/{n}"] = p_
            params[f"{part}/{n}".replace(".augmenter.noise_dist.", ".slicer.noise_dist.")] = p_
    worst, worst_name = 0.0, ""
    for key in names:
        assert params[key].grad is not None, key
        g = params[key].grad.double().cpu().reshape(-1)
        r = torch.from_numpy(synth.normal("gradproj/" + key, (g.numel(),), 0))
        got = np.concatenate([[g.sum().item(), g.abs().sum().item(), (g * r).sum().item()], np.pad(g[:HEAD].numpy(), (0, max(0, HEAD - g.numel())))])
        want = z["train/" + key]
        err = np.abs(got - want).max() / max(want[1], 1e-4 * gnorm)          # (floor: tensors whose exact gradient is zero hold rounding noise only)
        if err > worst:
            worst, worst_name = err, key
    moved = (bn1.running_mean - bn1_mean_before).abs().max().item()
    print(f"{case} (train mode): loss {loss.item():.6f} (ref {float(z['train/loss']):.6f}); d extract_1 rel err {dx_err:.1e}; {len(names)} parameter "
          f"gradients (embedder + flow), worst error / L1 norm {worst:.1e} ({worst_name}); bn1 running mean moved by {moved:.2e}")
    assert dx_err < 5e-4 and worst < 1e-3 and moved > 0
    md["flow"].eval()
    md["input_embedder"].eval()


# ---------------------------------------------------------------- two ranks on the card: sharded step + bucketed gradient all-reduce
def _sharded_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from flowcompare_amd import shard
        fx = Fixture("e2e_tiny_affine")                       # 3 scenes: uneven split 2 + 1
        cfg, md = _build(fx)
        md["flow"].train()                                    # embedder stays in eval(): BatchNorm batch statistics would be per shard
        reducer = shard.GradientReducer(md["flow"].parameters(), bucket_bytes=64 << 10)
        batch = tuple(None if t is None else t.to(DEV) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
        loss, lp, bpd, norm = shard.sharded_training_step(batch, md, cfg, reducer, optimizer=None, eps=[e.to(DEV) for e in fx.eps()], grad_clip=0)
        grads = {n: p.grad.detach().cpu().double().numpy() for n, p in md["flow"].named_parameters() if p.grad is not None}
        q.put((rank, float(loss), lp.shape[0], grads))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_sharded_training_step_matches_reference_full_batch_gradients():
    """Two processes on the one card (gloo): each differentiates its scenes (2 + 1) through the HIP training path, the bucketed SUM
    all-reduce runs from the backward hooks, and both ranks end with the flow gradients the reference's loss.backward() produced for
    the FULL batch (tests/golden/grad_tiny_affine.npz, eval record: the embedder is frozen here)."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    world = 2
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    procs = [ctxm.Process(target=_sharded_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=500) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    z = np.load(os.path.join(GOLDEN, "grad_tiny_affine.npz"))
    gnorm = float(z["eval/grad_norm"])
    assert [r[2] for r in res] == [2, 1]
    worst = 0.0
    for rank, loss, _, grads in res:
        assert abs(loss - float(z["eval/loss"])) < 2e-4 * abs(float(z["eval/loss"]))
        for key in json.loads(bytes(z["names_json"]).decode())["eval"]:
            if not key.startswith("flow/"):
                continue
            g = torch.from_numpy(grads[key.split("/", 1)[1]]).reshape(-1)
            r = torch.from_numpy(synth.normal("gradproj/" + key, (g.numel(),), 0))
            got = np.array([g.sum().item(), g.abs().sum().item(), (g * r).sum().item()])
            want = z["eval/" + key]
            worst = max(worst, np.abs(got - want[:3]).max() / max(want[1], 1e-4 * gnorm))
    for k in res[0][3]:
        assert np.array_equal(res[0][3][k], res[1][3][k])      # identical reduced gradients on both ranks
    print(f"two ranks, 2 + 1 scenes: worst flow-gradient error / L1 norm vs the reference's full-batch backward {worst:.1e}")
    assert worst < 1e-4


@pytest.mark.parametrize("name", ["e2e_tiny_FullCombiner", "e2e_tiny_ExponentialCombiner", "e2e_tiny_expcoupling", "e2e_tiny_expcoupling_orig"])
def test_flow_backward_with_dense_combiners_matches_oracle_autograd(name):
    """FullCombiner / ExponentialCombiner between the layers (models/permuters.py:15-53: weights built in parameter space, applied by
    the training Linear) and ExponentialCoupling (per-point matrix exponential, reverse mode through the Taylor-action recurrence):
    gradients (incl. w and the tanh-rescale scalars) against fp64 autograd through the pinned oracle."""
    fx = Fixture(name)
    cfg, md = _build(fx)
    loss, lp, x, ctx = _train_step(fx, cfg, md)
    c = fx.derived_cfg()
    sd_f, _ = fx.state_dicts(torch.float64)
    for v in sd_f.values():
        if v.is_floating_point():
            v.requires_grad_(True)
    e1 = fx.t("extract_1", torch.float64)[:, :, :c["input_dim"]].requires_grad_(True)
    ex = fx.t("extra", torch.float64)
    ex = None if ex is None else ex[:, None, :].expand(-1, e1.shape[1], -1)
    lp_o = O.flow_log_prob(c, sd_f, e1, ctx.detach().cpu().double(), ex, fx.eps(torch.float64))
    (-lp_o.mean()).backward()
    gn = sum(float((v.grad ** 2).sum()) for v in sd_f.values() if v.is_floating_point() and v.grad is not None) ** 0.5
    worst, worst_name = 0.0, ""
    for n, p in md["flow"].named_parameters():
        if sd_f[n].grad is None:
            continue
        e = (p.grad.double().cpu() - sd_f[n].grad).abs().sum().item() / max(sd_f[n].grad.abs().sum().item(), 1e-4 * gn)
        if e > worst:
            worst, worst_name = e, n
    print(f"{name}: loss diff {abs(loss.item() + lp_o.mean().item()):.1e} dx {_rel(x.grad, e1.grad):.1e}; worst parameter gradient L1 error {worst:.1e} ({worst_name})")
    assert abs(loss.item() + lp_o.mean().item()) < 2e-4 * max(1.0, abs(lp_o.mean().item())) and _rel(x.grad, e1.grad) < 5e-4 and worst < 1e-3


def test_five_adam_steps_follow_the_oracle_trajectory():
    """train.py's loop body (inner_loop -> backward -> clip_grad_norm_ -> Adam) for five steps on the HIP path, embedder and flow in
    train mode, against the same five steps of the pinned oracle under fp64 autograd with the same optimiser: the loss trajectory
    and the parameters after the last step."""
    fx = Fixture("e2e_tiny_affine")
    cfg, md = _build(fx)
    md["flow"].train()
    md["input_embedder"].train()
    cfg = dict(cfg)
    cfg["grad_clip_val"] = 5.0
    batch = tuple(None if t is None else t.to(DEV) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
    eps = [e.to(DEV) for e in fx.eps()]
    opt = torch.optim.Adam(md["parameters"], lr=2e-3)
    # the oracle side: same weights as leaf tensors, same Adam, same clipping
    c = fx.derived_cfg()
    sd_f, sd_e = fx.state_dicts(torch.float64)
    import re
    opt_leaves = []                                  # exactly the tensors that are nn.Parameters in the module mirror (bn{i} = conv{i}.1)
    for part, sd in (("flow", sd_f), ("input_embedder", sd_e)):
        for n, p_ in md[part].named_parameters():
            alias = re.sub(r"^bn(\d)\.", r"conv\1.1.", n)
            opt_leaves.append(sd[alias].requires_grad_(True))
    opt_o = torch.optim.Adam(opt_leaves, lr=2e-3)
    b64 = (fx.t("extract_0", torch.float64), fx.t("extract_1", torch.float64), fx.t("extra", torch.float64))
    losses_h, losses_o = [], []
    for step in range(5):
        loss, _, _, _ = TF.training_step(batch, md, cfg, optimizer=opt, eps=eps)
        losses_h.append(loss.item())
        opt_o.zero_grad(set_to_none=True)
        with O.train_mode():
            lo, _, _ = O.inner_loop(c, sd_f, sd_e, b64, fx.eps(torch.float64))
        lo.backward()
        torch.nn.utils.clip_grad_norm_([v for v in opt_leaves if v.grad is not None], max_norm=5.0)
        opt_o.step()
        losses_o.append(lo.item())
    worst, diffs = 0.0, []
    for part, sd in (("flow", sd_f), ("input_embedder", sd_e)):
        for n, p_ in md[part].named_parameters():
            alias = re.sub(r"^bn(\d)\.", r"conv\1.1.", n)
            d = (p_.detach().cpu().double() - sd[alias].detach()).abs().max().item()
            diffs.append((d, part + "/" + n))
            worst = max(worst, d)
    print("largest parameter differences:", [(f"{d:.1e}", n) for d, n in sorted(diffs, reverse=True)[:3]])
    print("loss trajectory HIP   : " + " ".join(f"{v:.5f}" for v in losses_h))
    print("loss trajectory oracle: " + " ".join(f"{v:.5f}" for v in losses_o) + f"   max parameter difference after 5 steps {worst:.1e}")
    assert losses_h[-1] < losses_h[0]
    assert max(abs(a - b) for a, b in zip(losses_h, losses_o)) < 1e-5 * abs(losses_o[0])
    assert worst < 1e-3
    md["flow"].eval()
    md["input_embedder"].eval()


def test_full_training_step_is_bit_reproducible():
    """Two runs of the whole train-mode step (embedder with batch-statistics BatchNorm + flow) give bit-identical gradients: every
    reduction of the backward has a fixed order, the EdgeConv input gradient included (owner-computes gather over the edges sorted by
    target instead of atomics)."""
    fx = Fixture("e2e_spline_L2")
    cfg, md = _build(fx)
    md["flow"].train()
    md["input_embedder"].train()
    batch = tuple(None if t is None else t.to(DEV) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
    eps = [e.to(DEV) for e in fx.eps()]
    runs = []
    for _ in range(2):
        for m in (md["flow"], md["input_embedder"]):
            m.zero_grad()
        with T.step_guard(device=DEV) as guard:
            loss, _, _ = fa.inner_loop(batch, md, cfg, eps=eps)
            loss.backward()
            assert not guard.overflowed()
        runs.append({f"{part}/{n}": p.grad.clone() for part in ("flow", "input_embedder") for n, p in md[part].named_parameters() if p.grad is not None})
    assert len(runs[0]) > 90 and all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    md["flow"].eval()
    md["input_embedder"].eval()


@pytest.mark.parametrize("case", ["tiny_spline_relu", "tiny_cif"])
def test_kept_and_recomputed_layers_give_the_same_bits(case):
    """The keep-or-checkpoint decision moves time, not numbers: without checkpointing (every layer keeps its activations), with an
    activation budget of 0 (every layer recomputed in backward) and of 1 byte (the first layer kept, the rest recomputed) the log-prob,
    d loss / d x, d loss / d context and every flow parameter's gradient are bit for bit the same (eval mode, inputs that require grad)."""
    fx = Fixture("e2e_" + case)
    cfg, md = _build(fx)
    runs = []
    for flow_kw in (dict(checkpoint=False), dict(activation_budget_bytes=0), dict(activation_budget_bytes=1)):
        loss, lp, x, ctx = _train_step(fx, cfg, md, **flow_kw)
        runs.append(dict({"flow/" + n: p.grad.clone() for n, p in md["flow"].named_parameters() if p.grad is not None},
                         log_prob=lp.detach().clone(), dx=x.grad.clone(), dctx=ctx.grad.clone()))
    assert len(runs[0]) > 10 and torch.isfinite(runs[0]["log_prob"]).all() and runs[0]["dx"].abs().max().item() > 0
    for other in runs[1:]:
        assert sorted(other) == sorted(runs[0])
        differ = [k for k in runs[0] if not torch.equal(runs[0][k], other[k])]
        assert not differ, differ


# ---------------------------------------------------------------- first batch under sharding: global ActNorm statistics, live parameters
def _sharded_init_worker(rank, world, port, q, backend):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if backend == "nccl":
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(DEV))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        from flowcompare_amd import shard
        fx = Fixture("e2e_tiny_affine")                       # 3 scenes: uneven split 2 + 1 when world == 2
        cfg, md = _build(fx)
        md["flow"].train()
        for m in md["flow"].modules():
            if hasattr(m, "initialized"):
                m.initialized.zero_()
        reducer = shard.GradientReducer(md["flow"].parameters(), bucket_bytes=64 << 10)
        before = {n: p for n, p in md["flow"].named_parameters()}
        opt = torch.optim.Adam(reducer.params, lr=1e-3)
        batch = tuple(None if t is None else t.to(DEV) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
        loss, lp, bpd, norm = shard.sharded_training_step(batch, md, cfg, reducer, optimizer=None, eps=[e.to(DEV) for e in fx.eps()], grad_clip=0)
        same_objects = all(p is before[n] for n, p in md["flow"].named_parameters())
        stats = {}
        for n, m in md["flow"].named_modules():
            if hasattr(m, "initialized"):
                assert float(m.initialized) == 1.0
                stats[n + ".shift"] = m.shift.detach().cpu().double().numpy()
                stats[n + ".log_scale"] = m.log_scale.detach().cpu().double().numpy()
                assert m.shift.grad is not None and m.log_scale.grad is not None      # live: reduced gradients reach the ActNorm parameters
        # a second step with the optimizer: parameters move identically on every rank
        shard.sharded_training_step(batch, md, cfg, reducer, optimizer=opt, eps=[e.to(DEV) for e in fx.eps()], grad_clip=1.0)
        digest = float(sum(p.detach().double().sum() for p in md["flow"].parameters()))
        unused = [n for n, p in md["flow"].named_parameters() if p.grad is None]
        q.put((rank, float(loss), same_objects, stats, digest, unused))
    finally:
        dist.destroy_process_group()


def _spawn(worker, world, *extra, timeout=500):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    procs = [ctxm.Process(target=worker, args=(r, world, port, q) + extra) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=timeout) for _ in range(world)), key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()                                      # exact child processes of this test only
    return res, [p.exitcode for p in procs]


@pytest.mark.timeout(900)
def test_two_rank_first_batch_actnorm_init_uses_global_statistics_and_keeps_parameters_live():
    """with un-initialised ActNorm layers the sharded step must not leave the ranks with different models.  Two ranks
    (2 + 1 scenes): the data-dependent initialisation all-reduces its column statistics, so both ranks land on the statistics the
    REFERENCE computed on the full batch in its first training forward (grad_tiny_affine.npz, record "init"), written in place (the
    reducer's and the optimizer's parameters stay the module's parameters), and a following Adam step moves both replicas identically."""
    res, codes = _spawn(_sharded_init_worker, 2, "gloo")
    assert codes == [0, 0]
    z = np.load(os.path.join(GOLDEN, "grad_tiny_affine.npz"))
    worst = 0.0
    for rank, loss, same_objects, stats, digest, unused in res:
        assert same_objects
        assert abs(loss - float(z["init/loss"])) < 2e-4 * max(1.0, abs(float(z["init/loss"])))
        for k, v in stats.items():
            want = z["init/" + k]
            worst = max(worst, np.abs(v - want).max() / max(1.0, np.abs(want).max()))
    assert worst < 1e-4
    for k in res[0][3]:
        assert np.array_equal(res[0][3][k], res[1][3][k])      # bit-identical ActNorm weights on both ranks
    assert res[0][4] == res[1][4]                               # and bit-identical parameters after the Adam step
    print(f"two ranks, first batch: ActNorm statistics of the GLOBAL batch, worst error vs the reference's first forward {worst:.1e}; "
          f"parameters without gradient (grad None on every rank): {res[0][5][:4]}")


@pytest.mark.timeout(900)
def test_sharded_training_step_over_rccl():
    """The same sharded step with backend "nccl" (= RCCL) and one rank: the collectives, the flat gradient views and the stream ordering
    are RCCL's (first-batch ActNorm init with all-reduced statistics, bucketed gradient all-reduce, presence mask, Adam step)."""
    res, codes = _spawn(_sharded_init_worker, 1, "nccl")
    assert codes == [0] and res[0][2]
    z = np.load(os.path.join(GOLDEN, "grad_tiny_affine.npz"))
    assert abs(res[0][1] - float(z["init/loss"])) < 2e-4 * max(1.0, abs(float(z["init/loss"])))
    # Two RCCL ranks on ONE device: tried on this pool (round 2) -- init_process_group hangs until the timeout, RCCL does not share a
    # device between ranks -- so the two-rank runs of the same code use gloo (the two tests above) and RCCL with > 1 rank is left to the
    # driver's 8-GPU node (bench.py --gpus N [--train]).


def test_training_step_rolls_back_a_rejected_fp16_attempt():
    """when the split-fp16 attempt leaves the fp16 range the step is repeated on the fp32-input loops; the rejected attempt
    must not leave traces: BatchNorm running statistics are updated once, from finite values, and the gradients equal those of a step
    that ran on the fp32-input loops from the start."""
    fx = Fixture("e2e_tiny_affine")
    cfg, md = _build(fx)
    md["flow"].train()
    md["input_embedder"].train()
    e0, e1, ex = fx.t("extract_0").to(DEV), fx.t("extract_1").to(DEV), fx.t("extra")
    e0 = e0.clone()
    e0[0, 0, 0] = 7.0e4                                              # a context coordinate outside the fp16 range: the guard flag rises in the
    batch = (e0, e1, None if ex is None else ex.to(DEV))             # embedder's first EdgeConv product; BatchNorm brings the features back to O(1)
    eps = [e.to(DEV) for e in fx.eps()]
    bn = md["input_embedder"].bn1
    rm0, nb0 = bn.running_mean.clone(), int(bn.num_batches_tracked)
    loss, lp, bpd, norm = TF.training_step(batch, md, cfg, optimizer=None, eps=eps, grad_clip=0)
    assert torch.isfinite(loss) and torch.isfinite(norm)
    g_retry = {n: p.grad.clone() for n, p in md["flow"].named_parameters() if p.grad is not None}
    rm_retry = bn.running_mean.clone()
    assert int(bn.num_batches_tracked) == nb0 + 1 and torch.isfinite(rm_retry).all()
    # the same step on the fp32-input loops only, from the same starting state
    with torch.no_grad():
        bn.running_mean.copy_(rm0)
    for m in md["input_embedder"].modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.num_batches_tracked.fill_(nb0)
    md["flow"].zero_grad(); md["input_embedder"].zero_grad()
    with T.step_guard(fp16=False, device=DEV):
        loss2, _, _ = fa.inner_loop(batch, md, cfg, eps=eps)
        loss2.backward()
    assert torch.equal(bn.running_mean, rm_retry)
    for n, p in md["flow"].named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, g_retry[n]), n
    md["flow"].eval(); md["input_embedder"].eval()


def _flat_adam_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from flowcompare_amd import shard
        torch.manual_seed(5)
        shapes = [(300, 512), (512,), (7,), (4097,), (64, 3, 1, 1), (1, 300)]
        ps = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]
        ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        reducer = shard.GradientReducer(ps, bucket_bytes=256 << 10)              # several buckets
        opt = shard.FlatAdam(reducer, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
        topt = torch.optim.Adam(ref, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
        worst_n = 0.0
        for it in range(4):
            reducer.zero_grad()
            gs = [torch.randn(s, device=DEV) * (10.0 if it == 1 else 0.1) for s in shapes]
            for p, r, g in zip(ps, ref, gs):
                p.grad.copy_(g)
                r.grad = g.clone()
            tn = torch.nn.utils.clip_grad_norm_(ref, max_norm=1.0)
            topt.step()
            n = opt.step(max_norm=1.0)
            worst_n = max(worst_n, abs(float(n) - float(tn)) / float(tn))
        err = max(float((p.detach() - r.detach()).abs().max()) for p, r in zip(ps, ref))
        sd = opt.state_dict()
        tsd = topt.state_dict()
        merr = max(float((sd["state"][j]["exp_avg"] - tsd["state"][j]["exp_avg"]).abs().max()) for j in range(len(ps)))
        # a resumed run: a fresh FlatAdam restored from torch's checkpoint layout (load_flow's optimizer entry), then one step in which
        # parameter 2 has no gradient on any rank -- torch.optim.Adam skips it (no weight decay, no moment decay), and so must the kernel
        opt2 = shard.FlatAdam(reducer, lr=1.0)
        opt2.load_state_dict(tsd)
        assert opt2.t == 4 and opt2.lr == 3e-3 and opt2.weight_decay == 0.01
        # (i) a parameter whose storage was replaced (module.to(), a re-created Parameter): the pointer table follows it
        ps[0].data = ps[0].data.clone()
        ref0 = ref[0].detach().clone()
        reducer.zero_grad()
        for p, r in zip(ps, ref):
            g = torch.randn(p.shape, device=DEV) * 0.1
            p.grad.copy_(g)
            r.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(ref, max_norm=1.0)
        topt.step()
        opt2.step(max_norm=1.0)
        assert not torch.equal(ref[0].detach(), ref0)
        err = max(err, max(float((p.detach() - r.detach()).abs().max()) for p, r in zip(ps, ref)))
        # (ii) parameter 2 without a gradient (last: FlatAdam keeps ONE step counter, torch one per parameter, so a skipped parameter's
        # bias corrections would differ from torch's in any later step that updates it again)
        reducer.zero_grad()
        gs = [torch.randn(s, device=DEV) * 0.1 for s in shapes]
        for j, (p, r, g) in enumerate(zip(ps, ref, gs)):
            if j == 2:
                p.grad, r.grad = None, None
                continue
            p.grad.copy_(g)
            r.grad = g.clone()
        reducer.absent = [j == 2 for j in range(len(ps))]
        before = ps[2].detach().clone()
        torch.nn.utils.clip_grad_norm_([r for r in ref if r.grad is not None], max_norm=1.0)
        topt.step()
        opt2.step(max_norm=1.0)
        assert torch.equal(ps[2].detach(), before), "a parameter without a gradient must be skipped"
        err = max(err, max(float((p.detach() - r.detach()).abs().max()) for p, r in zip(ps, ref)))
        q.put((rank, err, worst_n, merr))
    finally:
        dist.destroy_process_group()


def test_flat_adam_matches_torch_adam_with_clipping():
    """The native optimiser step (global-norm clip + Adam on the reducer's flat buffers, csrc/train_optim.hip) against
    torch.nn.utils.clip_grad_norm_ + torch.optim.Adam over four steps, one of them clipped hard; moments exported in torch's layout;
    then a fresh FlatAdam restored with load_state_dict, a step with a gradient-less parameter (skipped like torch skips it) and a step
    after a parameter's storage moved."""
    res, codes = _spawn(_flat_adam_worker, 1)
    assert codes == [0]
    _, err, worst_n, merr = res[0]
    print(f"FlatAdam vs torch Adam after 4 + 2 steps (resumed): max |dp| {err:.2e}, gradient norm rel. error {worst_n:.1e}, exp_avg max diff {merr:.1e}")
    assert err < 2e-6 and worst_n < 1e-6 and merr < 1e-7
