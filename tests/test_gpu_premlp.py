"""The row-resident pre-attention kernel premlp_rows_kernel<ACT, KSIN, NLU> (csrc/premlp.hip) called alone through fc_debug_premlp_q_f32
(engine.op_premlp_q) and compared with the chain in fp64 on the host (tests/premlp_util.py): q = LayerNorm(mlp(x)) Wq^T I^-0.5 log2 e.

Gate: max |q - q64| <= 16 e32, e32 = the error of the same chain in plain fp32 torch on the CPU (premlp_util: where the 16 comes from;
tests/test_premlp_host.py: five planted faults miss it by more than 6 x 64).  Every path-0 call also checks that the range flag stayed down,
so that the q it judges came from the kernel and not from the repeat on the separate launches.

Which case runs which instantiation that launch_premlp can select (ACT: none 0, gelu 1, relu 2, elu 3, lrelu 4):
  <ACT, 5, 0>, the compile-time k loop (K_pad 160)     test_activations[150-*] for all five ACT; <1, 5, 0> also test_widths[132-*], [150-*],
                                                       test_row_counts[150-*], test_inner_width_48, test_paths, test_rows_are_independent[150],
                                                       test_neighbour_columns[150], test_range_flag_from_an_input[150], the second call of
                                                       test_pre_layer_random; <2, 5, 0> also test_range_flag_from_a_hidden_activation
  <ACT, 0, 0>, the run-time k loop                     test_activations[90-*] for all five ACT (K_pad 96: 3-bit swizzle, general piece -> row map);
                                                       <1, 0, 0> also test_widths at K_pad 32, 96, 224 (3-bit swizzle), 64, 128, 192 (4-bit) and 256
                                                       (the cpr == 64 arm of pr_dma), test_row_counts[90-*], test_rows_are_independent[90],
                                                       test_neighbour_columns[20], [90], [190], test_range_flag_from_an_input[90]
_run asserts the instantiation's name from the in-library profiler's report of the call.
  <1, 5, 10>, with the ActNorm + LU pre-layer          test_pre_layer_exact_on_integers, test_pre_layer_random

Measured on an MI355X, worst max |q - q64| / e32 over all path-0 cases of this file:  plain 1.29 (the one-row case at k_in 150; 0.5 .. 0.9 at
300 rows and more),  flat 0.83  (paths 1 and 2: 0.86 and 0.75).  No case comes near the gate, and every bit-for-bit equality holds."""
import pytest
import torch

import premlp_util as PU
from flowcompare_amd import engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FC_ERR_UNSUPPORTED = 6


def _fallbacks():
    return engine.lib().fc_debug_fp16_fallbacks()


def _call(x, sd, act, path, k_in=None):
    """engine.op_premlp_q with the in-library profiler on: (result, names of the kernels the call launched).  Which path and which
    instantiation a call took is asserted from these, not assumed."""
    engine.profile_enable(True)
    engine.profile_reset()
    try:
        out = engine.op_premlp_q(None, sd, act, path, xprev=x) if "lu.weight" in sd else engine.op_premlp_q(x, sd, act, path, k_in=k_in)
        torch.cuda.synchronize()
        names = [r["kernel"] for r in engine.profile_report()]
    finally:
        engine.profile_enable(False)
        engine.profile_reset()
    return out, names


def _instantiation(sd, act):
    k_pad = (sd["net.in_layer.weight"].shape[1] + 31) // 32 * 32
    return f"premlp_rows_kernel<{engine.OP_ACTS[act]}, {5 if k_pad == 160 else 0}, {10 if 'lu.weight' in sd else 0}>"


def _run(c, path=0, x=None, sd=None, k_in=None):
    """q (and xnext) of case c on `path`.  The call must not have been repeated (on path 0 its q would be the separate launches'), and must
    have launched what the path names: on path 0 the expected instantiation of the kernel and no GEMM, on the others no premlp kernel."""
    before = _fallbacks()
    sd = c.sd if sd is None else sd
    out, names = _call((c.x if x is None else x).to(DEV), sd, c.act, path, k_in)
    assert _fallbacks() == before, f"{c.label()}: the range flag was raised on in-range inputs"
    ran = lambda s: any(s in n for n in names)
    if path == 0:
        assert ran(_instantiation(sd, c.act)) and not ran("gemm") and not ran("layernorm") and not ran("lnq_finalize"), names
    else:
        assert not ran("premlp") and ran("lnq_finalize_kernel") == (path == 1) and ran("layernorm_kernel") == (path == 2), names
    return out


def _gate(c, q, what="path 0"):
    r = c.ratio(q)
    print(f"{c.label()}, {what}: max |q - q64| / e32 = {r:.2f}   (e32 {c.e32:.2e}, max |q64| {c.q64.abs().max():.2f}, min row std {c.row_std_min:.3f})")
    assert r <= PU.GATE, f"{c.label()}, {what}: {r:.1f} e32"
    return r


@pytest.mark.parametrize("family", PU.FAMILIES)
@pytest.mark.parametrize("k_in", PU.WIDTHS)
def test_widths(k_in, family):
    """x1 widths 20 .. 256: K_pad 32, 64, 96, 128, 160, 160, 192, 224, 256 -- both swizzle masks on the run-time k loop, its cpr == 64 arm, and the
    compile-time arm at 160."""
    c = PU.case(k_in, 300, "gelu", family)
    _gate(c, _run(c))


@pytest.mark.parametrize("act", PU.ACT_NAMES)
@pytest.mark.parametrize("k_in", (150, 90))
def test_activations(k_in, act):
    c = PU.case(k_in, 300, act, "plain")
    _gate(c, _run(c))


@pytest.mark.parametrize("rows", (1, 127, 129, 515))
@pytest.mark.parametrize("k_in", (150, 90))
def test_row_counts(k_in, rows):
    """Around one 128-row workgroup; 515 rows are six workgroups after the padding to 256."""
    c = PU.case(k_in, rows, "gelu", "plain")
    _gate(c, _run(c))


def test_inner_width_48():
    """I = 48 pads to the kernel's 64 q columns: q comes back [rows, 48] and correct, the pad columns stay inside."""
    c = PU.case(150, 300, "gelu", "plain", inner=48)
    q = _run(c)
    assert tuple(q.shape) == (300, 48)
    _gate(c, q)


@pytest.mark.parametrize("family", PU.FAMILIES)
@pytest.mark.parametrize("k_in", (150, 90))
def test_paths(k_in, family):
    """The kernel, the LayerNorm -> q fold GEMM behind separate hidden layers, and separate launches throughout: each against fp64 with the
    same gate.  Their mutual differences are printed, not asserted: three arithmetics."""
    c = PU.case(k_in, 300, "gelu", family)
    q = [_run(c, path).cpu().double() for path in (0, 1, 2)]
    for path in (0, 1, 2):
        _gate(c, q[path], f"path {path}")
    print(f"{c.label()}: max |path 0 - 1| {(q[0] - q[1]).abs().max():.2e}  |0 - 2| {(q[0] - q[2]).abs().max():.2e}  |1 - 2| {(q[1] - q[2]).abs().max():.2e}")


@pytest.mark.parametrize("k_in", (150, 90))
def test_rows_are_independent(k_in):
    """A point's q must not depend on its lane, wave or workgroup, nor on the slice of the scratch its residual was parked in: a permutation of
    700 rows permutes q bit for bit, rows 37..299 alone give the same bits, and so does a second call."""
    c = PU.case(k_in, 700, "gelu", "plain")
    full = _run(c).cpu()
    _gate(c, full)
    perm = torch.randperm(700, generator=torch.Generator().manual_seed(3))
    assert torch.equal(_run(c, x=c.x[perm]).cpu(), full[perm])
    assert torch.equal(_run(c, x=c.x[37:300]).cpu(), full[37:300])
    assert torch.equal(_run(c).cpu(), full), "the row-resident kernel is not deterministic"


@pytest.mark.parametrize("k_in", (20, 90, 150, 190))
def test_neighbour_columns(k_in):
    """The engine's latent has the first x2 columns behind x1 inside the padded width; the packed in_layer is zero there.  Random finite values in
    columns k_in .. K_pad - 1 give the q of zeros there, bit for bit."""
    c = PU.case(k_in, 300, "gelu", "plain")
    kp = (k_in + 31) // 32 * 32
    wide = torch.zeros(300, kp)
    wide[:, :k_in] = c.x
    q0 = _run(c, x=wide, k_in=k_in).cpu()
    assert torch.equal(q0, _run(c).cpu())
    wide[:, k_in:] = PU.make_input(300, kp - k_in, seed=77) * 10.0
    assert torch.equal(_run(c, x=wide, k_in=k_in).cpu(), q0)


def _out_of_range(c, x, sd):
    """One call that must be repeated once on the bf16 limbs: q finite and within 1e-5 (1 + |q64|) of fp64 (the relative gate of
    test_split_fp16_out_of_range_falls_back_to_bf16_limbs)."""
    q64, h = PU.q_ref64(x, sd, c.act)
    assert h.std(-1, unbiased=False).min().item() > PU.MIN_ROW_STD
    before = _fallbacks()
    q, names = _call(x.to(DEV), sd, c.act, 0)
    q = q.cpu().double()
    assert _fallbacks() == before + 1
    # the kernel raised the flag itself (nothing else ran in front of it), and the repeat took the separate launches
    assert any(_instantiation(sd, c.act) in n for n in names) and any("layernorm_kernel" in n for n in names), names
    rel = ((q - q64).abs() / (1 + q64.abs())).max().item()
    print(f"{c.label()}: repeated on the bf16 limbs, max |q - q64| / (1 + |q64|) = {rel:.2e}")
    assert torch.isfinite(q).all() and rel < 1e-5


@pytest.mark.parametrize("k_in", (150, 90))
def test_range_flag_from_an_input(k_in):
    """The kernel's own range flag: an in-range call adds nothing to fc_debug_fp16_fallbacks (every _run checks that), one input of 1e5 adds 1."""
    c = PU.case(k_in, 300, "gelu", "plain")
    _run(c)
    x = c.x.clone()
    x[17, 5] = 1.0e5
    _out_of_range(c, x, c.sd)


def test_range_flag_from_a_hidden_activation():
    """Inputs in range, but the in_layer's bias drives one hidden activation past 65504 under RELU: only the epilogue's amax can see it."""
    c = PU.case(150, 300, "relu", "plain")
    sd = dict(c.sd)
    sd["net.in_layer.bias"] = sd["net.in_layer.bias"].clone()
    sd["net.in_layer.bias"][7] = 7.0e4
    _out_of_range(c, c.x, sd)


@pytest.mark.parametrize("rows", (300, 129))
def test_pre_layer_exact_on_integers(rows):
    """<GELU, 5, 10>: integer-valued xprev, lu.weight and lu.bias in [-8, 8] make every partial sum of the 320-wide pre-layer exact, so xnext
    must equal xprev W^T + b bit for bit -- any fragment, swizzle or chunk-order mistake shows.  (The in_layer is scaled down so that the
    integers' large latent stays inside fp16's range through the chain: the xnext judged is the kernel's.)"""
    c = PU.case(150, rows, "gelu", "plain", lu_dim=300)
    g = torch.Generator().manual_seed(11 + rows)
    ri = lambda *sh: torch.randint(-8, 9, sh, generator=g).float()
    sd = dict(c.sd)
    sd["lu.weight"], sd["lu.bias"], xprev = ri(300, 300), ri(300), ri(rows, 300)
    sd["net.in_layer.weight"] = sd["net.in_layer.weight"] * 1e-3
    q, xnext = _run(c, x=xprev, sd=sd)
    assert torch.isfinite(q).all() and tuple(xnext.shape) == (rows, 300)
    assert torch.equal(xnext.cpu(), xprev @ sd["lu.weight"].t() + sd["lu.bias"])


@pytest.mark.parametrize("rows", (300, 129))
def test_pre_layer_random(rows):
    """<GELU, 5, 10> on random operands: xnext within test_linear_matches_fp64's bound 2e-6 sqrt(K); q within the gate of the fp64 chain over
    the fp64 xnext; and q equal, bit for bit, to the q of the kernel without the pre-layer fed the returned xnext -- the same fp32 values
    split into the same limbs meet the same MFMAs in the same order."""
    c = PU.case(150, rows, "gelu", "plain", lu_dim=300)
    q, xnext = _run(c)
    err = (xnext.cpu().double() - c.xnext64).abs().max().item()
    print(f"{c.label()}: max |xnext - fp64| {err:.2e}")
    assert err < 2e-6 * 300 ** 0.5
    _gate(c, q, "path 0 with the pre-layer")
    sd = {k: v for k, v in c.sd.items() if not k.startswith("lu.")}
    q_plain = _run(c, x=xnext[:, :150].contiguous(), sd=sd)
    assert torch.equal(q_plain.cpu(), q.cpu()), f"max |q - q(without the pre-layer)| {(q_plain - q).abs().max().item():.2e}"
    for path in (1, 2):
        qp, xp = _run(c, path)
        _gate(c, qp, f"path {path} with the map as its own GEMM")
        assert (xp.cpu().double() - c.xnext64).abs().max().item() < 2e-6 * 300 ** 0.5


def _refused(match, x, sd, act="gelu", xprev=None):
    with pytest.raises(engine.FcError, match=match) as err:
        engine.op_premlp_q(x, sd, act, 0, xprev=xprev)
    assert err.value.code == FC_ERR_UNSUPPORTED


def test_path_0_refuses_what_the_kernel_does_not_take():
    """path 0 runs the row-resident kernel or fails with FC_ERR_UNSUPPORTED and a message that names the condition; it never takes another
    path.  The I = 32 model that path 0 refuses matches fp64 on path 2."""
    x150 = PU.make_input(300, 150, seed=5).to(DEV)
    c32 = PU.case(150, 300, "gelu", "plain", inner=32)
    _refused(r"premlp_fusable.*inner width I = 32", c32.x.to(DEV), c32.sd)
    _gate(c32, _run(c32, 2), "path 2")
    sd = PU.make_state(150, seed=1, n_mid=3)
    _refused(r"premlp_fusable.*3 hidden layers", x150, sd)
    sd = PU.make_state(150, seed=2, hidden=128)
    _refused(r"premlp_fusable.*hidden width 128", x150, sd)
    sd = PU.make_state(300, seed=3)
    _refused(r"premlp_fusable.*k_in pads to 320", PU.make_input(300, 300, seed=6).to(DEV), sd)
    sd = PU.make_state(100, seed=4, lu_dim=200)
    _refused(r"premlp_lu_fusable.*D = 200", None, sd, xprev=PU.make_input(300, 200, seed=7).to(DEV))
    sd = PU.make_state(150, seed=5, lu_dim=300)
    _refused(r"premlp_lu_fusable.*GELU only", None, sd, act="relu", xprev=PU.make_input(300, 300, seed=8).to(DEV))
