"""ExponentialCoupling training backward at 17 <= d2 <= 160 (fc_train_expm_wide_bwd_f32, csrc/expm_wide.hip; opt-in through
config['expm_wide_backward']): the operator against fp64 autograd through torch.matrix_exp, bit stability and row independence, the
norm bound, the argument checks, the reference fixtures through the training path, and one training step at the shipped width."""
import pytest
import torch

import flowcompare_amd as fa
from flowcompare_amd import engine
from flowcompare_amd import modules as M
from flowcompare_amd import train_flow as TF
from flowcompare_amd import train_ops as T
from flowcompare_amd.conditioning import condition_flow
from conftest import Fixture
from fullsize_util import synth_pairs
from oracle import flow_oracle as O
from test_expm_wide_bwd_host import autograd_reference, make_case, make_w, SCAL4
from test_gpu_train import _rel, _train_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FC_ERR_INVALID = 1
ROWS = 5


def _up(n, m=32):
    return (n + m - 1) // m * m


def _panels(raw, x2, b, dy2, rows_pad=None):
    """The operator's padded inputs on the device: o = [d2*d2 raw | d2 shift b] at pitch round_up(d2*d2 + d2, 32), x2 and dy2 at
    round_up(d2, 32); rows_pad: zero rows up to the panel height the autograd node asks for."""
    rows, d2 = x2.shape
    rp = rows_pad or rows
    o = torch.zeros(rp, _up(d2 * d2 + d2), device=DEV)
    o[:rows, :d2 * d2] = raw.reshape(rows, -1).to(DEV)
    o[:rows, d2 * d2:d2 * d2 + d2] = b.to(DEV)
    xp, dyp = torch.zeros(rp, _up(d2), device=DEV), torch.zeros(rp, _up(d2), device=DEV)
    xp[:rows, :d2], dyp[:rows, :d2] = x2.to(DEV), dy2.to(DEV)
    return o, xp, dyp


def _vec(v, rows_pad):
    out = torch.zeros(rows_pad, device=DEV)
    out[:v.shape[0]] = v.to(DEV)
    return out


def _run(o, xp, dyp, dldj, scal4, d2, rows=None):
    """One call of the C entry; outputs start as garbage so that every element the kernel must write is seen.  Returns (code, dx2, dout,
    dscal, status)."""
    rows = o.shape[0] if rows is None else rows
    dx2 = torch.full_like(xp, 7.0)
    dout = torch.full_like(o, 7.0)
    dscal = torch.full((o.shape[0], 4), 7.0, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    try:
        code = engine.lib().fc_train_expm_wide_bwd_f32(engine._ptr(xp), xp.shape[1], engine._ptr(o), o.shape[1], engine._ptr(scal4), engine._ptr(dyp),
                                                       dyp.shape[1], engine._ptr(dldj), engine._ptr(dx2), dx2.shape[1], engine._ptr(dout), dout.shape[1],
                                                       engine._ptr(dscal), rows, d2, engine._ptr(status), engine._stream())
    except engine.FcError as e:                                    # the binding raises on a status; the tests below look at the code
        code = e.code
    torch.cuda.synchronize()
    return code, dx2.cpu(), dout.cpu(), dscal.cpu(), int(status.item())


@pytest.mark.parametrize("norm", [0.01, 0.3, 4.0, 32.0])
@pytest.mark.parametrize("d2", [17, 32, 33, 64, 65, 128, 129, 150, 160])
def test_operator_matches_fp64_autograd(d2, norm):
    """dx2 and the d raw block: max |g - g64| / max |g64| <= 2e-6 (the fp32 restatement of the recurrence in
    tests/test_expm_wide_bwd_host.py is 3e-8 .. 6.6e-7; the margin covers the kernel's tree-order sums and tanhf).  d b = dy2 bit for bit, pad columns 0.
    The four scalar gradients are sums of rows d2^2 products: |v - v64| <= 4 E with E = max(|v32 - v64|, 4 2^-24 sum |terms64|), v32 eager
    fp32 torch on the CPU."""
    raw, x2, b, dy2, dldj, scal4 = make_case(d2, norm, ROWS, seed=d2)
    ref = autograd_reference(raw, x2, b, dy2, dldj, scal4, torch.float64)
    e32 = autograd_reference(raw, x2, b, dy2, dldj, scal4, torch.float32)
    o, xp, dyp = _panels(raw, x2, b, dy2)
    code, dx2, dout, dscal, status = _run(o, xp, dyp, dldj.to(DEV), scal4.to(DEV), d2)
    assert code == 0 and status == 0
    np_ = d2 * d2 + d2
    ex, er = _rel(dx2[:, :d2], ref["dx2"], 0.0), _rel(dout[:, :d2 * d2], ref["draw"].reshape(ROWS, -1), 0.0)
    ex32, er32 = _rel(e32["dx2"], ref["dx2"], 0.0), _rel(e32["draw"].reshape(ROWS, -1), ref["draw"].reshape(ROWS, -1), 0.0)
    v, v64, v32 = dscal.double().sum(0), ref["dscal"], e32["dscal"].double()
    E = torch.maximum((v32 - v64).abs(), 4 * 2.0 ** -24 * ref["terms"])
    ratio = (v - v64).abs() / E
    print(f"d2 {d2} ||W||_1 {norm}: dx2 {ex:.1e} (eager fp32 {ex32:.1e}) draw {er:.1e} (eager fp32 {er32:.1e}); dscal |v - v64| / E "
          + " ".join(f"{float(r):.2f}" for r in ratio))
    assert torch.equal(dout[:, d2 * d2:np_], dy2)
    assert (dx2[:, d2:] == 0).all() and (dout[:, np_:] == 0).all()
    assert ex <= 2e-6 and er <= 2e-6
    assert (ratio <= 4.0).all()


@pytest.mark.parametrize("d2,norm", [(33, 32.0), (150, 4.0)])
def test_bit_stable_and_row_independent(d2, norm):
    raw, x2, b, dy2, dldj, scal4 = make_case(d2, norm, ROWS, seed=3)
    o, xp, dyp = _panels(raw, x2, b, dy2)
    dl, s4 = dldj.to(DEV), scal4.to(DEV)
    first = _run(o, xp, dyp, dl, s4, d2)
    second = _run(o, xp, dyp, dl, s4, d2)
    assert first[0] == 0 and first[4] == 0
    assert all(torch.equal(a, c) for a, c in zip(first[1:4], second[1:4]))
    pick = [1, 3]
    sub = _run(o[pick].contiguous(), xp[pick].contiguous(), dyp[pick].contiguous(), dl[pick].contiguous(), s4, d2)
    assert sub[0] == 0 and all(torch.equal(a, c[pick]) for a, c in zip(sub[1:4], first[1:4]))


def _bound_case():
    d2, bad = 33, 2
    raw, x2, b, dy2, dldj, scal4 = make_case(d2, [4.0, 0.3, 600.0, 4.0, 32.0], ROWS, seed=9)
    return d2, bad, raw, x2, b, dy2, dldj, scal4


def test_norm_beyond_the_bound_raises_the_status_word():
    """One row at ||A||_1 ~ 600 > 40 theta_55 = 534 among normal rows: status raised, that row NaN, the other rows as without it."""
    d2, bad, raw, x2, b, dy2, dldj, scal4 = _bound_case()
    A = make_w(d2, [4.0, 0.3, 600.0, 4.0, 32.0], ROWS, seed=9)[bad]
    A = A - torch.diagonal(A).mean() * torch.eye(d2, dtype=A.dtype)
    assert float(A.abs().sum(0).max()) > 540.0
    o, xp, dyp = _panels(raw, x2, b, dy2)
    code, dx2, dout, dscal, status = _run(o, xp, dyp, dldj.to(DEV), scal4.to(DEV), d2)
    assert code == 0 and status == 1
    np_ = d2 * d2 + d2
    assert torch.isnan(dx2[bad, :d2]).all() and torch.isnan(dout[bad, :np_]).all() and torch.isnan(dscal[bad]).all()
    assert (dx2[bad, d2:] == 0).all() and (dout[bad, np_:] == 0).all()
    good = [r for r in range(ROWS) if r != bad]
    alone = _run(o[good].contiguous(), xp[good].contiguous(), dyp[good].contiguous(), dldj[good].to(DEV), scal4.to(DEV), d2)
    assert alone[0] == 0 and alone[4] == 0
    assert torch.equal(alone[1], dx2[good]) and torch.equal(alone[2], dout[good]) and torch.equal(alone[3], dscal[good])


def test_autograd_node_turns_the_status_into_a_runtime_error():
    d2, bad, raw, x2, b, dy2, dldj, scal4 = _bound_case()
    o, xp, dyp = _panels(raw, x2, b, dy2, T.ROW_PAD)
    s4 = scal4.to(DEV)
    with pytest.raises(RuntimeError, match="exceeds the matrix-exponential kernel's bound"):
        T.ExpmCouplingFn.apply(xp, o, s4, ROWS, d2, True)
    # the backward's own status: the saved panel leaves the bound between the forward and the backward
    o_ok = o.clone()
    o_ok[bad] = o[0]
    o_ok.requires_grad_(True)
    y2, ldj = T.ExpmCouplingFn.apply(xp, o_ok, s4, ROWS, d2, True)
    o_ok.data[bad] = o[bad]
    with pytest.raises(RuntimeError, match=r"training backward\).*exceeds the matrix-exponential kernel's bound"):
        torch.autograd.backward([y2, ldj], [dyp, _vec(dldj, T.ROW_PAD)])


@pytest.mark.parametrize("d2", [16, 161])
def test_c_entry_refuses_widths_outside_17_to_160(d2):
    rows = 2
    o = torch.zeros(rows, _up(d2 * d2 + d2), device=DEV)
    xp = torch.zeros(rows, _up(d2), device=DEV)
    code, dx2, dout, dscal, status = _run(o, xp, xp.clone(), torch.zeros(rows, device=DEV), torch.tensor(SCAL4, device=DEV), d2)
    assert code == FC_ERR_INVALID and status == 0
    assert (dx2 == 7.0).all() and (dout == 7.0).all()            # nothing was launched


def test_autograd_node_refuses_d2_above_160_after_a_successful_forward():
    d2, rows = 200, 2
    raw, x2, b, dy2, dldj, scal4 = make_case(d2, 0.3, rows, seed=1)
    o, xp, dyp = _panels(raw, x2, b, dy2, T.ROW_PAD)
    o.requires_grad_(True)
    y2, ldj = T.ExpmCouplingFn.apply(xp, o, scal4.to(DEV), rows, d2, True)
    assert torch.isfinite(y2).all()
    with pytest.raises(RuntimeError, match="supports d2 <= 160"):
        torch.autograd.backward([y2, ldj], [dyp, _vec(dldj, T.ROW_PAD)])
    assert o.grad is None


@pytest.mark.parametrize("name", ["e2e_expwide_d20", "e2e_expwide_d21_orig", "e2e_expwide_L2"])
def test_flow_backward_at_wide_d2_matches_oracle_autograd(name):
    """The reference fixtures at d2 = 20, 21 and 150 through the training path with expm_wide_backward on: procedure and gates of
    test_gpu_train.py::test_flow_backward_with_dense_combiners_matches_oracle_autograd (fp64 autograd through the pinned oracle)."""
    fx = Fixture(name)
    cfg = dict(fx.cfg)
    cfg["expm_wide_backward"] = True
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    sd_flow, sd_emb = fx.state_dicts()
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
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


def test_training_step_at_the_shipped_width():
    """C4 with flow_type ExponentialCoupling (d2 = 150), 3 layers, conditioned weights: one Adam step."""
    N = 256
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", sample_size=N, n_flow_layers=3, flow_type="ExponentialCoupling", expm_wide_backward=True)
    torch.manual_seed(11)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    nz = cfg["latent_dim"] - cfg["input_dim"]
    c0, c1, cx, ce = synth_pairs(2, N, N, 999, nz)
    condition_flow(md, cfg, (c0.to(DEV), c1.to(DEV), cx.to(DEV)), eps=[ce.to(DEV)])
    md["flow"].train()
    couplings = [m for m in md["flow"].modules() if isinstance(m, M.ExponentialCoupling)]
    assert len(couplings) == 3 and couplings[0].input_dim - couplings[0].split_dim == 150
    watched = {}
    for i, cp in enumerate(couplings):
        watched[f"{i}.out_layer.weight"] = cp.nn.out_layer.weight
        for n in ("scale", "shift", "rescale", "reshift"):
            watched[f"{i}.{n}"] = getattr(cp, n)
    before = {n: p.detach().clone() for n, p in watched.items()}
    opt = torch.optim.Adam(md["parameters"], lr=1e-3)
    e0, e1, extra, eps = synth_pairs(2, N, N, 6, nz)
    grads = {}                                                   # the state of every .grad when Adam steps (training_step clears them after)

    def record(optimizer, args, kwargs):
        for n, p in md["flow"].named_parameters():
            if p.requires_grad:
                grads[n] = p.grad is not None and bool(torch.isfinite(p.grad).all())

    hook = opt.register_step_pre_hook(record)
    try:
        loss, lp, bpd, norm = TF.training_step((e0.to(DEV), e1.to(DEV), extra.to(DEV)), md, cfg, optimizer=opt, eps=[eps.to(DEV)])
    finally:
        hook.remove()
        md["flow"].eval()
    print(f"d2 = 150 training step: loss {float(loss):.4f} grad norm {float(norm):.3e}")
    assert torch.isfinite(loss) and torch.isfinite(norm)
    assert grads and all(grads.values()), [n for n, ok in grads.items() if not ok]
    unchanged = [n for n, p in watched.items() if torch.equal(p.detach(), before[n])]
    assert not unchanged, unchanged
