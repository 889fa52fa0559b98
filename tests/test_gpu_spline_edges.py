"""The spline evaluators of csrc/spline.h on knots, the +-3 boundary and floor bins, through the envelope checker of tests/spline_edge_util.py
(R, the parameter families, the fp32 oracle's residuals and the tolerance rule are recorded in that module's docstring; every tolerance here
is 3 x the fp32 oracle's residual + a floor, or a sum of such).

Op level: engine.op_rqspline (rq_spline_elem via rq_any) at K = 4, 8, 16, forward and inverse, every family, and the round trip.  Inverse: every
family is gated; single elements at which the reference's quadratic loses its digits in fp32 are left out by an fp64 criterion
(spline_edge_util.inverse_error_estimate; tests/test_spline_edges_host.py pins how many), and the kernel may return no NaN anywhere.

Fused evaluators (rq_spline_fwd_regs in its four callers): a crafted two-layer c2 flow puts exact inputs and exact parameters at layer 0's
evaluator.  The augmenter's out_layer is zero (mean 0, scale exp(0) = 1), so the latent is [x | eps] and layer 0's x2 is eps[..., d1 - 6:]
bit for bit (asserted on the engine's trace); layer 0's coupling net has a zero out_layer weight and the chosen parameters as its bias; the
ActNorm and LinearLU between the layers are the identity (zero shift, zero log-scale, zero off-diagonal entries, a diagonal parameter whose
softplus + eps rounds to 1.0f), so layer 1's traced x2 is layer 0's y element by element.  Layer 1 keeps lively random parameters; its
inside / outside decisions are forced on the oracle from the HIP trace (tests/fullsize_util.py).
  * y: element-wise through the checker.  It has been through the identity LU GEMM, so an outside element's |y - x| is gated like any residual
    (op level holds the bit-for-bit rule; here log|det| == 0 outside shows in the row sums).
  * log|det|: a row's log-prob against [lo, hi] = the fp64 oracle's row log-prob with every layer-0 element's log|det| replaced by its
    envelope's minimum / maximum; tolerance = the sum of the row's element tolerances (150 x the family's in a one-family run) + the fp32
    oracle's worst row residual of everything but the layer-0 spline, measured the same way.
Runs per configuration: one per family (all dims carry it; row r of scene 0 carries edge input r, scene 1 the list reversed) and a mixed one
(dim j carries family j mod 7: the parameter-column layout, the fifth-dim lane transposition and the ragged last tile with edge values in them).

Findings recorded by these tests (MI355X):
  * Bit identity: knob 13 = 2 and 13 = 4 give equal y and log-prob bits on all 8 runs.  13 = 5 with 34 = 0 gives the y bits of 13 = 4 on all 8 runs
    and, on rows with one live dim (where a tile's log-det sum is exact), its log-prob bits too: the claim of rq_spline_fwd_regs's header
    (the scaled form rounds exactly like the unscaled one) HOLDS.  On dense rows its log-probs differ from 13 = 4's by 1.8e-4 .. 4.9e-4
    (a few ulps of sums near -500: the wide kernel adds a tile's five log-dets in another order, and layer 1's parameters come out of
    another GEMM arithmetic); the code nowhere claims those bits.
  * Both ends of the wide kernel's weight exponent hold: a zero weight (wmax == 0, exponent 0) and 1e-30 randn (exponent at its cap of 100)
    pass every gate with the same residuals.
  * Three kernel faults found and fixed in csrc/spline.h (before the fix these tests missed by the figures given):
    - 16 bins, family "flat bin between knots beyond 10" (15 equal bins 0.033 wide beside one 5.5 wide), forward, BOTH evaluators: op_rqspline
      y residual 2.17e-5 (tol 2.06e-5), log|det| 7.27e-4 (tol 2.49e-4); fused / unfused flow y 2.18e-5, row log-prob 1.09e-1 (tol 3.84e-2).
      The kernels added the 16 softmax terms and the 16 bin sizes one by one in fp32, and fifteen equal addends round the same way at every
      step: the width knots sat 8.6 units of 2^-22 from their fp64 places (a plain fp32 restatement with exact exponentials shows the
      same), outside the R = 4 envelope, and mid-bin y was off by 3.6e-5 where the fp32 oracle is off by 2e-7 (ATen's CPU cumsum accumulates
      float in double).  Now summed in blocks of four at 16 bins (rq_prefix): 2.5 units on this family.  K <= 8 keeps its chain and its bits.
    - Round trip at K = 8, family "lively": |lad_inv + lad_fwd| 1.37e-3 (fp32 oracle 1.52e-4, tol 9.57e-4) for y just below height knot 1,
      where dy/dx = 0.034.  The quadratic's root came out as 1.0000045 (its discriminant, 0.005, is a difference of two numbers near 189):
      the point left the bin by 3e-6 while log|det| was still taken from the bin's own formula.  The root is now held at 1.
    - Inverse: the discriminant is (h d1)^2 at a bin's upper knot, taken as a difference of numbers of order one; where it rounded below zero
      the kernel returned NaN (3 elements of "ramps + softplus switch" at K = 16; the fp32 oracle does on 6 of "floor bins at both ends" at
      K = 8).  It is now held at zero: the kernel returns no NaN inside the domain, which the op-level test asserts.
"""
import contextlib
import functools
import io
import math

import pytest
import torch

import flowcompare_amd as fa
import spline_edge_util as SU
from flowcompare_amd import engine
from fullsize_util import hip_rows_with_trace
from knob_util import knobs
from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N, M = 2, 300, 64
LIVELY = 3.0                   # tests/test_gpu_spline_fold.py: scale of layer 1's parameter layer
AUG, L0, ACTNORM, LU, L1 = "transforms.0.augment.noise_dist.net", "transforms.1.transform.nn", "transforms.2", "transforms.3", "transforms.4.transform.nn"


def _name(K, inverse):
    return f"K {K} {'inverse' if inverse else 'forward'}"


# ---------------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("K", SU.BINS)
def test_op_rqspline_on_knots_boundary_and_floor_bins(K, inverse):
    c = SU.case(K, inverse)
    y, lad = engine.op_rqspline(c["x"].to(DEV), c["p"].float().to(DEV), K, inverse=inverse)
    y, lad = y.cpu(), lad.cpu()
    nan = torch.isnan(y) | torch.isnan(lad)
    print(f"op_rqspline {_name(K, inverse)}: {c['x'].numel()} elements; NaN from the kernel on {int(nan.sum())}, from the fp32 oracle on "
          f"{int((torch.isnan(c['y32']) | torch.isnan(c['lad32'])).sum())}")
    assert SU.check(f"op_rqspline {_name(K, inverse)}", c, y, lad) == []
    assert not nan.any()                       # (the inverse holds a discriminant that rounds below zero at zero: csrc/spline.h)


@pytest.mark.parametrize("K", SU.BINS)
def test_op_rqspline_round_trip(K):
    """forward(inverse(y)) against y and lad_inv + lad_fwd at the recovered point, as tests/test_gpu_ops.py::test_spline_golden_forward_and_inverse
    does, on the elements spline_edge_util.round_trip keeps (its docstring says which are left out and why; tests/test_spline_edges_host.py pins
    how many are kept), every family: 3 x the fp32 oracle's own round trip + that test's gates."""
    c, rt = SU.case(K, True), SU.round_trip(K)
    p = c["p"].float().to(DEV)
    xi, li = engine.op_rqspline(c["x"].to(DEV), p, K, inverse=True)
    y2, l2 = engine.op_rqspline(xi, p, K)
    assert SU.report(f"round trip K {K}", c["names"], c["fam"], rt["err"](y2.cpu() - c["x"]), rt["err"]((l2 + li).cpu()), rt["gates"]) == []


# ---------------------------------------------------------------------------------------------------------------- the crafted flow
def _identity_diag(eps):
    """the fp32 diagonal parameter u of LinearLU for which softplus(u) + eps, taken in fp64 as the engine's pack and the oracle take it,
    rounds to 1.0f: the folded ActNorm + LU weight is then the identity matrix exactly"""
    u = torch.tensor(math.log(math.expm1(1.0 - eps)), dtype=torch.float32)
    up = dn = u
    for _ in range(5):
        for v in (up, dn):
            if float((torch.nn.functional.softplus(v.double()) + eps).float()) == 1.0:
                return float(v)
        up, dn = torch.nextafter(up, torch.tensor(math.inf)), torch.nextafter(dn, torch.tensor(-math.inf))
    raise AssertionError("no fp32 diagonal parameter gives softplus(u) + eps == 1.0f")


@functools.lru_cache(maxsize=None)
def _base(K, latent_dim):
    """config, the crafted state dict (layer 0's bias still to be set per run) and the inputs of one configuration: made once, never modified"""
    cfg = fa.named_config("c2_dgcnn_attn_spline", n_flow_layers=2, sample_size=N, latent_dim=latent_dim, cif_latent_dim=latent_dim, num_bins_spline=K)
    torch.manual_seed(100 + K + latent_dim)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device="cpu", mode="test")
    sd = {k: v.detach().clone() for k, v in md["flow"].state_dict().items()}
    sd_e = {k: v.detach().clone() for k, v in md["input_embedder"].state_dict().items()}
    for k in (f"{AUG}.out_layer.weight", f"{AUG}.out_layer.bias", f"{L0}.out_layer.weight", f"{ACTNORM}.shift", f"{ACTNORM}.log_scale", f"{LU}.lower_entries", f"{LU}.upper_entries"):
        sd[k] = torch.zeros_like(sd[k])
    sd[f"{ACTNORM}.initialized"] = torch.ones_like(sd[f"{ACTNORM}.initialized"])
    sd[f"{LU}.unconstrained_upper_diag"] = torch.full_like(sd[f"{LU}.unconstrained_upper_diag"], _identity_diag(cfg["linear_lu_eps"]))
    for k in (f"{L1}.out_layer.weight", f"{L1}.out_layer.bias"):
        sd[k] = sd[k] * LIVELY
    g = torch.Generator().manual_seed(200 + K + latent_dim)
    d1 = latent_dim // 2
    x, ctx = torch.rand(B, N, cfg["input_dim"], generator=g), torch.randn(B, M, cfg["input_embedding_dim"], generator=g)
    eps = torch.randn(B, N, latent_dim - cfg["input_dim"], generator=g)
    w30 = 1e-30 * torch.randn(sd[f"{L0}.out_layer.weight"].shape, generator=g)
    return dict(cfg=cfg, sd=sd, sd_e=sd_e, x=x, ctx=ctx, eps=eps, d1=d1, d2=latent_dim - d1, K=K, w30=w30, inputs=SU.flow_inputs(K, B, N))


def _runs(base):
    """[(name, family of every transformed dim)]: one run per family, then the mixed one"""
    F = len(base["inputs"]["names"])
    return [(name, torch.full((base["d2"],), f)) for f, name in enumerate(base["inputs"]["names"])] + [("mixed", torch.arange(base["d2"]) % F)]


def _crafted(base, fam_of_dim, tiny_weight=False):
    """(state dict, noise) of one run: layer 0's parameters in its bias in the reference's [d2][3K+1] order, its inputs in the noise"""
    K, c = base["K"], base["inputs"]
    sd = dict(base["sd"])
    params = torch.stack([p for _, p in SU.families(K)])[fam_of_dim]                       # [d2, 3K+1]
    sd[f"{L0}.out_layer.bias"] = params.float().reshape(-1)
    if tiny_weight:
        sd[f"{L0}.out_layer.weight"] = base["w30"]
    eps = base["eps"].clone()
    eps[..., base["d1"] - base["cfg"]["input_dim"]:] = c["X"][fam_of_dim].permute(1, 2, 0)   # [B, N, d2]
    return sd, eps


def _oracle_rows(base, sd, eps, dtype, forced):
    """the oracle's Flow.log_prob [B, N] with the spline decisions `forced` (None = its own), and the decisions it used"""
    sdt = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad(), O.spline_decisions(forced) as rec:
        lp = O.flow_log_prob(base["cfg"], sdt, base["x"].to(dtype), base["ctx"].to(dtype), None, [eps.to(dtype)])
    return lp.double(), [m.clone() for m in rec]


_ORACLE = {}


def _reference(base, run, tiny_weight, dec_hip):
    """What a run is gated against, cached per run and per set of decisions (the variants of one configuration share it): the element tables of
    the run's x2, the row envelope [lo, hi] of the fp64 oracle under the HIP run's decisions, and the row tolerance."""
    name, fam_of_dim = _runs(base)[run]
    key = (base["K"], base["d2"], run, tiny_weight)
    if key not in _ORACLE:
        sd, eps = _crafted(base, fam_of_dim, tiny_weight)
        lp32, dec32 = _oracle_rows(base, sd, eps, torch.float32, None)
        _ORACLE[key] = dict(sd=sd, eps=eps, lp32=lp32, dec32=dec32, lp64={})
    o = _ORACLE[key]

    def lp64(dec):
        k = b"".join(m.numpy().tobytes() for m in dec)
        if k not in o["lp64"]:
            o["lp64"][k] = _oracle_rows(base, o["sd"], o["eps"], torch.float64, dec)[0]
        return o["lp64"][k]
    c = base["inputs"]
    BN = B * N
    idx = (fam_of_dim[None, :] * BN + torch.arange(BN)[:, None]).reshape(B, N, -1)                   # element (b, r, j) in the tables of c
    take = lambda t: t[idx]
    lad64, lad32 = take(c["flad64"]), take(c["lad32"].double())
    lo = lp64(dec_hip) - lad64.sum(-1) + take(c["env"][2]).sum(-1)
    hi = lp64(dec_hip) - lad64.sum(-1) + take(c["env"][3]).sum(-1)
    # everything but the layer-0 spline, fp32 oracle against fp64 under the fp32 run's own decisions
    rest32 = float(((o["lp32"] - lad32.sum(-1)) - (lp64(o["dec32"]) - lad64.sum(-1))).abs().max())
    tol_row = float(torch.tensor(c["direct"]["tol_lad"], dtype=torch.float64)[fam_of_dim].sum()) + rest32
    # the fp32 oracle's own row residual, for the log
    ref_row = float(torch.maximum(lo - o["lp32"], o["lp32"] - hi).clamp_min(0).max()) if all(torch.equal(a, b) for a, b in zip(dec_hip, o["dec32"])) else float("nan")
    return dict(idx=idx, lo=lo, hi=hi, tol_row=tol_row, rest32=rest32, ref_row=ref_row, fam=fam_of_dim[None, None, :].expand(B, N, -1))


@functools.lru_cache(maxsize=None)
def _module(K, latent_dim, fold):
    """a module on the device whose flow is packed under knob 34 = fold (the knob is read when a flow is packed)"""
    with knobs({34: fold}), contextlib.redirect_stdout(io.StringIO()):
        return fa.initialize_flow(_base(K, latent_dim)["cfg"], device=DEV, mode="test")


def _hip(base, sd, eps, settings):
    """(log-prob [B, N], traced x2 [2, B, N, d2]) of the HIP flow on one run under the knob settings"""
    fold = settings.get(34, 1)
    md = _module(base["K"], base["d2"] + base["d1"], fold)
    with knobs({**settings, 34: fold}):
        fa.load_flow({"flow": sd, "input_embedder": base["sd_e"]}, md)
        return hip_rows_with_trace(base["cfg"], md, base["ctx"].to(DEV), base["x"], None, [eps])


def _check_run(label, base, run, settings, tiny_weight=False):
    """One run under one variant through every gate; returns (log-prob, layer-1 trace) for the bit-identity tests."""
    c = base["inputs"]
    name, fam_of_dim = _runs(base)[run]
    sd, eps = _crafted(base, fam_of_dim, tiny_weight)
    lp, trace = _hip(base, sd, eps, settings)
    x2 = eps[..., base["d1"] - base["cfg"]["input_dim"]:]
    # (equal as numbers = bit for bit up to the sign of the one -0.0 input, which mean + eps * scale = 0 + -0 * 1 turns into +0)
    assert torch.equal(trace[0], x2), f"{label} {name}: layer 0's x2 is not the noise bit for bit"
    dec = [(t >= -3.0) & (t <= 3.0) for t in trace]
    ref = _reference(base, run, tiny_weight, dec)
    # y, element by element: the trace of layer 1 against the envelope times the LU diagonal (1 to 2e-8 in the oracle's fp64)
    dg = float(O.lu_matrices({k: v.double() for k, v in sd.items() if k.startswith(LU)}, LU, base["cfg"]["linear_lu_eps"])[2][0])
    env = tuple(t[ref["idx"]].reshape(-1) * dg for t in c["env"][:2]) + (None, None)
    ry, = SU.residuals(x2.reshape(-1), None, base["K"], trace[1].reshape(-1), None, env=env, exact_outside=False)
    fam = ref["fam"].reshape(-1)
    row = torch.maximum(ref["lo"] - lp.double(), lp.double() - ref["hi"]).clamp_min(0.0)
    row = torch.where(torch.isnan(lp), torch.full_like(row, math.inf), row)
    failed = []
    for f in sorted(set(fam_of_dim.tolist())):
        wy = float(ry[fam == f].max())
        print(f"{label} | {name} | {c['names'][f]}: y residual {wy:.2e} (fp32 oracle {c['direct']['ref_y'][f]:.2e}, tol {c['direct']['tol_y'][f]:.2e})")
        if not wy <= c["direct"]["tol_y"][f]:
            failed.append(f"y of {c['names'][f]}")
    per_elem = float(row.max()) / base["d2"]
    print(f"{label} | {name}: row log-prob residual {float(row.max()):.2e} = {per_elem:.2e} per element (fp32 oracle row residual {ref['ref_row']:.2e}; tol {ref['tol_row']:.2e} = "
          f"sum of the row's element tolerances + {ref['rest32']:.2e} for the fp32 oracle's rest of the flow); {int((~dec[0]).sum())} / {int((~dec[1]).sum())} outside decisions in layer 0 / 1")
    if not float(row.max()) <= ref["tol_row"]:
        failed.append("row log-prob")
    assert failed == [], f"{label} | {name}: misses {failed}"
    return lp, trace[1]


SHIPPED, UNFOLDED, PERSISTENT, LDS_TILE, UNFUSED = {13: 5, 34: 1}, {13: 5, 34: 0}, {13: 4, 34: 0}, {13: 2, 34: 0}, {7: 0}
K8_VARIANTS = {"shipped (13 = 5, 34 = 1)": SHIPPED, "25-parameter image (34 = 0)": UNFOLDED, "persistent loop (13 = 4)": PERSISTENT,
               "LDS parameter tile (13 = 2)": LDS_TILE, "unfused (7 = 0)": UNFUSED}
N_RUNS = 8


@pytest.mark.parametrize("run", range(N_RUNS))
@pytest.mark.parametrize("variant", sorted(K8_VARIANTS))
def test_fused_evaluators_of_the_k8_layer(variant, run):
    base = _base(8, 300)
    assert len(_runs(base)) == N_RUNS
    _check_run(variant, base, run, K8_VARIANTS[variant])


@pytest.mark.parametrize("run", range(N_RUNS))
@pytest.mark.parametrize("variant", ["shipped (13 = 5, 34 = 1)", "25-parameter image (34 = 0)"])
def test_wide_kernel_with_two_live_dims_in_the_last_wave_tile(variant, run):
    _check_run(f"latent_dim 264, {variant}", _base(8, 264), run, K8_VARIANTS[variant])


@pytest.mark.parametrize("run", range(N_RUNS))
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("K", [4, 16])
def test_lds_tile_evaluator_at_4_and_16_bins(K, fused, run):
    _check_run(f"K {K}, knob 7 = {fused}", _base(K, 300), run, {7: fused})


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("run", range(N_RUNS))
def test_bit_identity_where_the_code_claims_it(run):
    """csrc/spline.h: ONE body serves every caller, so knob 13 = 2 and 13 = 4 give equal y and log-prob bits; and the scaled form (the wide
    kernel, 13 = 5) rounds exactly like the unscaled one, so with a zero weight (the parameters ARE the bias in every variant) the
    25-parameter image gives the y bits of 13 = 4 as well.  Its LOG-PROB bits cannot be compared on these runs: layer 1's parameters come out
    of another GEMM arithmetic, and the wide kernel adds a tile's five log-dets in another order (sw_row_sum, then dim 4); the difference is
    printed and held within 64 ulps of the batch's largest row sum, and the next test isolates the evaluator's log|det| bits."""
    base = _base(8, 300)
    name, fam_of_dim = _runs(base)[run]
    sd, eps = _crafted(base, fam_of_dim)
    out = {v: _hip(base, sd, eps, s) for v, s in (("13 = 4", PERSISTENT), ("13 = 2", LDS_TILE), ("13 = 5, 34 = 0", UNFOLDED))}
    lp4, y4 = out["13 = 4"][0], out["13 = 4"][1][1]
    for v in ("13 = 2", "13 = 5, 34 = 0"):
        lp, y = out[v][0], out[v][1][1]
        print(f"bit identity | {name} | {v} against 13 = 4: y trace {'equal' if _bits_equal(y, y4) else f'differs by up to {(y - y4).abs().max().item():.2e}'}, "
              f"log-prob {'equal' if _bits_equal(lp, lp4) else f'differs by up to {(lp - lp4).abs().max().item():.2e}'}")
        assert _bits_equal(y, y4), f"{name}: y of {v} and 13 = 4 differ by up to {(y - y4).abs().max().item():.2e}"
        # a pin against a gross regression of the dense rows: the ~60 tile partials of a row are added in another order, each addition good to
        # half an ulp of the running sum, which is of the size of the batch's largest |log-prob| even where the row's total is small: 64 ulps
        # of that bound it (measured: 8 ulps of 512 .. 1024)
        assert bool(((lp - lp4).abs() <= 64 * 2.0 ** -23 * float(lp4.abs().max())).all()), f"{name}: log-prob of {v} and 13 = 4 differ by up to {(lp - lp4).abs().max().item():.2e}"
    assert _bits_equal(out["13 = 2"][0], lp4), f"{name}: log-prob of 13 = 2 and 13 = 4 differ by up to {(out['13 = 2'][0] - lp4).abs().max().item():.2e}"


def test_log_det_bits_of_the_scaled_form_on_rows_with_one_live_dim():
    """The evaluator's log|det| bit for bit, 13 = 5 with 34 = 0 against 13 = 4 and 13 = 2: in row r only dim r mod d2 carries an edge input
    (family (r mod d2) mod 7), every other dim carries 3.5 (outside: y = x, log|det| = 0 exactly), and BOTH layers' out_layer weights are zero
    (their parameters are their biases in every variant).  A tile's log-det sum is then one value plus zeros, exact in any order, in both
    layers (layer 1 sees the same x2 through the identity LU), so equal log-prob bits are equal log|det| bits of the live elements."""
    base = _base(8, 300)
    c, d2 = base["inputs"], base["d2"]
    fam_of_dim = _runs(base)[-1][1]
    sd, eps = _crafted(base, fam_of_dim)
    sd[f"{L1}.out_layer.weight"] = torch.zeros_like(sd[f"{L1}.out_layer.weight"])
    x2 = torch.full((B, N, d2), 3.5)
    r = torch.arange(N)
    for b in range(B):
        x2[b, r, r % d2] = c["X"][fam_of_dim[r % d2], b, r]
    eps[..., base["d1"] - base["cfg"]["input_dim"]:] = x2
    out = {v: _hip(base, sd, eps, s) for v, s in (("13 = 4", PERSISTENT), ("13 = 2", LDS_TILE), ("13 = 5, 34 = 0", UNFOLDED))}
    live = int(((x2 >= -3) & (x2 <= 3)).sum())
    assert live > 0.9 * B * N                             # (a family's 22 inputs beyond +-3 are outside as well)
    for v in ("13 = 2", "13 = 5, 34 = 0"):
        same_lp, same_y = _bits_equal(out[v][0], out["13 = 4"][0]), _bits_equal(out[v][1][1], out["13 = 4"][1][1])
        print(f"bit identity | one live dim per row ({live} live elements) | {v} against 13 = 4: y {'equal' if same_y else 'DIFFERS'}, log-prob "
              f"{'equal' if same_lp else 'differs by up to %.2e' % (out[v][0] - out['13 = 4'][0]).abs().max().item()}")
        assert same_y and same_lp


@pytest.mark.parametrize("run", range(N_RUNS))
def test_shipped_kernel_with_the_weight_scale_at_its_cap(run):
    """A zero out_layer weight takes spline_wide_attach through its wmax == 0 branch (exponent 0: every other test of this file); weights of
    1e-30 put the exponent at its cap of 100."""
    _check_run("shipped, weights 1e-30 randn", _base(8, 300), run, SHIPPED, tiny_weight=True)
