"""The flow's element training operators one by one (csrc/train_rows.hip through train_ops.AffineFn / GaussDrawFn / NormalLogProbFn /
BaseDensityFn, csrc/train_expm.hip through ExpmCouplingFn and the C entries fc_train_expm_fwd_f32 / fc_train_expm_bwd_f32; csrc/train_wgrad.hip and train_linear.hip through
fc_train_colsum_f32, fc_train_act_fwd_f32 and fc_train_act_bwd_f32): forward and backward element-wise against the plain fp64 references
of tests/elem_ops_ref.py (pinned to the oracle by test_oracle_elem_ops.py).

Gate (embed_ops_ref.gate): per tensor err = max |hip - f64| / max(1e-2, max |f64|) < max(5e-6, 3 e32) with e32 the error of the same
reference run in eager fp32 on the CPU, measured in the test.  The loss is L = sum out dy + sum ldj dldj with random dy, dldj.  The clamp
of the std is discontinuous: every clamp case keeps each log std 1e-3 or more from log(clamp), with a quarter or more of the entries on
either side (asserted on the CPU).  The narrow ExponentialCoupling kernels: y2, dx2 and the d raw block within elem_ops_ref.expm_gate()
= max(2e-6, 3 x the error of the fp32 restatement of their recurrence, measured on the CPU) of fp64 autograd through torch.matrix_exp.
Outputs and gradients come from dirtied allocations (`_dirt`, which also checks that the allocator hands the dirt back): every pad column
of a valid row and every pad row must be exactly 0.

Kernel -> test (affine .. base: train_rows.hip; expm: train_expm.hip, arithmetic in expm_narrow.h; colsum: train_wgrad.hip; act: train_linear.hip):
  affine_train_fwd_kernel, affine_train_bwd_kernel   test_affine_matches_fp64 (exp and sigmoid; d scale and d shift apart)
  gauss_train_fwd_kernel, gauss_train_bwd_kernel     test_gauss_draw_matches_fp64 (clamp 0, 10, 0.5; odd eps pitch)
  normlp_train_fwd_kernel, normlp_train_bwd_kernel   test_normal_log_prob_matches_fp64 (clamp 0, 10, 0.5; v in a wider panel)
  base_train_fwd_kernel, base_train_bwd_kernel       test_base_density_matches_fp64
  expm_train_fwd_kernel, expm_train_bwd_kernel       test_expm_narrow_matches_fp64, test_expm_narrow_is_bit_stable_and_row_independent,
                                                     test_expm_coupling_node_matches_fp64 (ds4 through _colsum, pad rows),
                                                     test_expm_norm_beyond_32_raises_from_the_status_word, test_expm_bwd_refuses_d2_17
  colsum_kernel, colsum_reduce_kernel                test_colsum_matches_fp64 (scalar fallback, accumulate, 1 .. 256 splits)
  act_fwd_kernel, act_bwd_kernel                     test_standalone_activation_passes_match_fp64"""
import functools
import math
import types

import pytest
import torch

import elem_ops_ref as R
from flowcompare_amd import engine
from flowcompare_amd import train_ops as T
from test_gpu_train_embed_ops import DEV, JUNK_SEED, _pad, _panel, _zero

pytestmark = pytest.mark.gpu
FC_ERR_INVALID = 1


def _r32(n):
    return T._round_up(n, 32)


def _in(x2d, wide, junk, grad=True):
    """An input panel of a case: pitch round_up(width, 32), or 32 more with other data in the extra columns; pad rows 0 or junk."""
    width = x2d.shape[1]
    p = _panel(x2d, _r32(width) + (32 if wide else 0), junk)
    if wide:
        p[:x2d.shape[0], _r32(width):] = torch.randn(x2d.shape[0], 32, generator=torch.Generator().manual_seed(JUNK_SEED + 2)).to(DEV)
    return p.requires_grad_(grad)


def _up_grad(t2d, like, junk):
    """An upstream gradient for the panel `like`"""
    return _panel(t2d, like.shape[1], junk, rows_pad=like.shape[0])


def _up_vec(v, like, junk):
    out = torch.full((like.shape[0],), float(junk), device=DEV)
    out[:v.shape[0]] = v.to(DEV)
    return out


def _dirt(*shapes):
    """Leaves 7.0 in freed blocks of these shapes, so that an element a kernel skips shows; all are held at once, so two of one size are
    two blocks.  Then checks that the dirt arrives: fresh torch.empty of the same shapes, in the order in which the node under test asks
    for them next, read 7.0 everywhere (on the CPU: nothing else is allocated on the device before the node runs, so the node gets the
    same blocks).  Whatever else the test needs on the device is therefore built BEFORE this call."""
    held = [torch.full(s, 7.0, device=DEV) for s in shapes]
    del held
    got = [torch.empty(s, device=DEV) for s in shapes]
    arrived = [bool((t.cpu() == 7.0).all()) for t in got]
    del got
    assert all(arrived), f"the dirtied blocks {shapes} did not come back from the allocator: {arrived}"


def _pads(rows, **panels):
    """name -> (panel or vector, valid width): its pad rows and the pad columns of its valid rows"""
    out = {}
    for name, (t, width) in panels.items():
        out[name + " pad rows"] = t[rows:]
        if t.dim() == 2:
            out[name + " pad columns"] = t[:rows, width:]
    return out


def _assert_zero(tag, pads):
    bad = [what for what, t in pads.items() if not _zero(t)]
    assert not bad, f"{tag}: not exactly zero: {bad}"


@functools.lru_cache(maxsize=None)
def _case(table, name):
    """(case, fp64 reference, eager fp32 reference): computed once, shared by the tests, never written to."""
    make, refs = {"affine": (R.make_affine_case, R.affine_refs), "gauss": (R.make_gauss_case, R.gauss_refs),
                  "normlp": (R.make_normlp_case, R.normlp_refs), "base": (R.make_base_case, R.base_refs),
                  "expm": (R.make_expm_case, R.expm_refs)}[table]
    c = make(name)
    return c, refs(c, torch.float64), refs(c, torch.float32)


# ================================================================ affine coupling
def _run_affine(c):
    rows, d2 = c["rows"], c["d2"]
    x2, st = _in(c["x2"], c["wide"], c["junk"]), _in(c["st"], c["wide"], c["junk"])
    _dirt((x2.shape[0], _r32(d2)), (x2.shape[0],))
    y2, ldj = T.affine(x2, st, rows, d2, c["kind"])
    assert y2.shape == (_pad(rows), _r32(d2)) and ldj.shape == (_pad(rows),)
    ups = [_up_grad(c["dy2"], y2, c["junk"]), _up_vec(c["dldj"], ldj, c["junk"])]
    _dirt(tuple(x2.shape), tuple(st.shape))
    torch.autograd.backward([y2, ldj], ups)
    y2, ldj = y2.detach(), ldj.detach()
    assert x2.grad.shape == x2.shape and st.grad.shape == st.shape
    hip = dict(y2=y2[:rows, :d2], ldj=ldj[:rows], dx2=x2.grad[:rows, :d2], dscale=st.grad[:rows, :d2], dshift=st.grad[:rows, d2:2 * d2])
    return hip, _pads(rows, y2=(y2, d2), ldj=(ldj, 0), dx2=(x2.grad, d2), dst=(st.grad, 2 * d2))


@pytest.mark.parametrize("name", list(R.AFFINE_CASES))
def test_affine_matches_fp64(name):
    c, r64, r32 = _case("affine", name)
    raw = c["st"][:, :c["d2"]]
    assert (raw == -R.SATURATED).any() and torch.isfinite(r32["ldj"]).all()
    assert (raw == R.SATURATED).any() if c.get("high", True) else raw.max() <= 3.0
    hip, pads = _run_affine(c)
    R.gate(name, hip, r64, r32)
    _assert_zero(name, pads)
    assert torch.equal(hip["dshift"].cpu(), c["dy2"])                    # d shift is dy2 itself
    again, _ = _run_affine(c)
    assert all(torch.equal(hip[k], again[k]) for k in hip)


# ================================================================ the augmenter's Gaussian draw
def _run_gauss(c):
    rows, nz, clamp = c["rows"], c["nz"], c["clamp"]
    p = _in(c["p"], c["wide"], c["junk"])
    eps = c["eps"].to(DEV)                                              # dense [rows, nz] at pitch nz
    _dirt((p.shape[0], _r32(nz)), (p.shape[0],))
    z, ldj = T.gauss_draw(p, eps, rows, nz, clamp)
    assert z.shape == (_pad(rows), _r32(nz)) and ldj.shape == (_pad(rows),)
    ups = [_up_grad(c["dz"], z, c["junk"]), _up_vec(c["dldj"], ldj, c["junk"])]
    _dirt(tuple(p.shape))
    torch.autograd.backward([z, ldj], ups)
    z, ldj = z.detach(), ldj.detach()
    assert p.grad.shape == p.shape
    hip = dict(z=z[:rows, :nz], ldj=ldj[:rows], dmean=p.grad[:rows, :nz], dlogstd=p.grad[:rows, nz:2 * nz])
    return hip, _pads(rows, z=(z, nz), ldj=(ldj, 0), dp=(p.grad, 2 * nz))


def _clamped(c):
    return c["p"][:, c["nz"]:].double() > math.log(c["clamp"])


@pytest.mark.parametrize("name", list(R.GAUSS_CASES))
def test_gauss_draw_matches_fp64(name):
    c, r64, r32 = _case("gauss", name)
    hip, pads = _run_gauss(c)
    R.gate(name, hip, r64, r32)
    _assert_zero(name, pads)
    assert torch.equal(hip["dmean"].cpu(), c["dz"])                      # d mean is dz itself
    if c["clamp"] > 0:
        cl = _clamped(c)
        assert cl.any() and (~cl).any()
        assert (hip["dlogstd"].cpu()[cl] == 0).all(), f"{name}: a clamped entry has a log-std gradient"
        assert (hip["dlogstd"].cpu()[~cl] != 0).all()
    if c["clamp"] > 0:
        # ldj with log(clamp) at the clamped entries, not with their own log std.  Wherever the two differ by more than 1e-3 of max |ldj|
        # (every case of 32 columns or more; at 3 columns they can be close, and there the gate above is the check) the kernel's is 100
        # times closer to the first
        ls = c["p"][:, c["nz"]:].double()
        own = (0.5 * c["eps"].double() ** 2 + ls + R.HALF_LOG_2PI).sum(-1)
        want = (0.5 * c["eps"].double() ** 2 + torch.where(cl, torch.full_like(ls, math.log(c["clamp"])), ls) + R.HALF_LOG_2PI).sum(-1)
        apart = R.rel(own, r64["ldj"]) > 1e-3
        print(f"{name}: ldj with the clamped entries' own log std is {R.rel(own, r64['ldj']):.1e} from the reference")
        assert R.rel(want, r64["ldj"]) < 1e-12 and (apart or c["nz"] < 32)
        if apart:
            assert R.rel(hip["ldj"], want) < R.rel(hip["ldj"], own) * 1e-2
    again, _ = _run_gauss(c)
    assert all(torch.equal(hip[k], again[k]) for k in hip)


# ================================================================ the Slice log-density
def _run_normlp(c):
    rows, nz, clamp = c["rows"], c["nz"], c["clamp"]
    v, p = _in(c["v"], c["wide_v"], c["junk"]), _in(c["p"], c["wide"], c["junk"])
    _dirt((v.shape[0],))
    out = T.normal_log_prob(v, p, rows, nz, clamp)
    assert out.shape == (_pad(rows),)
    up = _up_vec(c["g"], out, c["junk"])
    _dirt(tuple(v.shape), tuple(p.shape))
    out.backward(up)
    out = out.detach()
    assert v.grad.shape == v.shape and p.grad.shape == p.shape
    hip = dict(out=out[:rows], dv=v.grad[:rows, :nz], dmean=p.grad[:rows, :nz], dlogstd=p.grad[:rows, nz:2 * nz])
    return hip, _pads(rows, out=(out, 0), dv=(v.grad, nz), dp=(p.grad, 2 * nz))


@pytest.mark.parametrize("name", list(R.NORMLP_CASES))
def test_normal_log_prob_matches_fp64(name):
    c, r64, r32 = _case("normlp", name)
    hip, pads = _run_normlp(c)
    R.gate(name, hip, r64, r32)
    _assert_zero(name, pads)
    assert torch.equal(hip["dmean"], -hip["dv"])
    if c["clamp"] > 0:
        cl = _clamped(c)
        assert cl.any() and (~cl).any()
        assert (hip["dlogstd"].cpu()[cl] == 0).all(), f"{name}: a clamped entry has a log-std gradient"
    again, _ = _run_normlp(c)
    assert all(torch.equal(hip[k], again[k]) for k in hip)


# ================================================================ the base density
def _run_base(c):
    rows, width = c["rows"], c["width"]
    x = _in(c["x"], c["wide"], c["junk"])
    _dirt((x.shape[0],))
    out = T.base_density(x, rows, width)
    assert out.shape == (_pad(rows),)
    up = _up_vec(c["g"], out, c["junk"])
    _dirt(tuple(x.shape))
    out.backward(up)
    out = out.detach()
    assert x.grad.shape == x.shape
    return dict(out=out[:rows], dx=x.grad[:rows, :width]), _pads(rows, out=(out, 0), dx=(x.grad, width))


@pytest.mark.parametrize("name", list(R.BASE_CASES))
def test_base_density_matches_fp64(name):
    c, r64, r32 = _case("base", name)
    if c["scale"] == "u30":
        assert c["x"].abs().max() > 29.9 and r64["out"].abs().max() > 4e4
    hip, pads = _run_base(c)
    R.gate(name, hip, r64, r32)
    _assert_zero(name, pads)
    again, _ = _run_base(c)
    assert all(torch.equal(hip[k], again[k]) for k in hip)


# ================================================================ ExponentialCoupling at d2 <= 16
SPARE = 3            # rows of every panel beyond `rows` in the C-entry tests: the kernels must leave them alone


def _run_expm(o, xp, dyp, dldj, scal4, d2, rows, forward=True):
    """fc_train_expm_fwd_f32 and fc_train_expm_bwd_f32 on outputs that start as 7.0.  Returns (code, dict of CPU tensors, status)."""
    L = engine.lib()
    t = dict(y2=torch.full_like(xp, 7.0), ldj=torch.full((o.shape[0],), 7.0, device=DEV), dx2=torch.full_like(xp, 7.0),
             dout=torch.full_like(o, 7.0), dscal=torch.full((o.shape[0], 4), 7.0, device=DEV))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    P = engine._ptr
    try:
        if forward:
            L.fc_train_expm_fwd_f32(P(xp), xp.shape[1], P(o), o.shape[1], P(scal4), P(t["y2"]), xp.shape[1], P(t["ldj"]), rows, d2, P(status),
                                    engine._stream())
        code = L.fc_train_expm_bwd_f32(P(xp), xp.shape[1], P(o), o.shape[1], P(scal4), P(dyp), dyp.shape[1], P(dldj), P(t["dx2"]), xp.shape[1],
                                       P(t["dout"]), o.shape[1], P(t["dscal"]), rows, d2, engine._stream())
    except engine.FcError as e:                                    # the binding raises on a status; the tests look at the code
        code = e.code
    torch.cuda.synchronize()
    return code, {k: v.cpu() for k, v in t.items()}, int(status.item())


def _panels(raw, x2, b, dy2, rows_pad=None):
    """The operator's padded inputs on the device: o = [d2*d2 raw | d2 shift b] at pitch round_up(d2*d2 + d2, 32), x2 and dy2 at
    round_up(d2, 32); rows_pad: zero rows beyond the case's."""
    rows, d2 = x2.shape
    rp = rows_pad or rows
    o, xp, dyp = torch.zeros(rp, _r32(d2 * d2 + d2)), torch.zeros(rp, _r32(d2)), torch.zeros(rp, _r32(d2))
    o[:rows, :d2 * d2], o[:rows, d2 * d2:d2 * d2 + d2] = raw.reshape(rows, -1), b
    xp[:rows, :d2], dyp[:rows, :d2] = x2, dy2
    return o.to(DEV), xp.to(DEV), dyp.to(DEV)


def _vec(v, rows_pad):
    out = torch.zeros(rows_pad)
    out[:v.shape[0]] = v
    return out.to(DEV)


def _expm_inputs(c, pick=None):
    rows = c["rows"] if pick is None else len(pick)
    sel = (lambda t: t) if pick is None else (lambda t: t[pick])
    o, xp, dyp = _panels(sel(c["raw"]), sel(c["x2"]), sel(c["b"]), sel(c["dy2"]), rows + SPARE)
    return o, xp, dyp, _vec(sel(c["dldj"]), rows + SPARE), c["scal4"].to(DEV), c["d2"], rows


@pytest.mark.parametrize("name", list(R.EXPM_CASES))
def test_expm_narrow_matches_fp64(name):
    """y2, dx2 and the d raw block: max |a - a64| / max |a64| <= elem_ops_ref.expm_gate() (4.2e-6 as measured by
    test_oracle_elem_ops.py::test_narrow_recurrence_in_fp32_against_fp64_autograd).  ldj = tr W under the row-kernel gate, d b = dy2 bit
    for bit, pad columns 0, rows beyond `rows` untouched.  The four scalar gradients are sums of rows d2^2 products:
    |v - v64| <= 4 E with E = max(|v32 - v64|, 4 2^-24 sum |terms64|), v32 eager fp32 torch on the CPU (tests/test_gpu_expm_wide_bwd.py)."""
    c, r64, r32 = _case("expm", name)
    d2, rows, np_ = c["d2"], c["rows"], c["d2"] * c["d2"] + c["d2"]
    code, t, status = _run_expm(*_expm_inputs(c))
    assert code == 0 and status == 0
    limit = R.expm_gate()
    cells, errs = [], {}
    for key, got, want in (("y2", t["y2"][:rows, :d2], "y"), ("dx2", t["dx2"][:rows, :d2], "dx2"), ("draw", t["dout"][:rows, :d2 * d2], "draw")):
        w64, w32 = r64[want].reshape(rows, -1), r32[want].reshape(rows, -1)
        errs[key] = R.rel(got, w64, 0.0)
        cells.append(f"{key} {errs[key]:.1e}/{R.rel(w32, w64, 0.0):.1e}")
    v, v64, v32 = t["dscal"][:rows].double().sum(0), r64["dscal"], r32["dscal"].double()
    E = torch.maximum((v32 - v64).abs(), 4 * 2.0 ** -24 * r64["terms"])
    ratio = (v - v64).abs() / E
    print(f"{name}: gate {limit:.1e}  err/e32  " + "  ".join(cells) + "  dscal |v - v64| / E " + " ".join(f"{float(r):.2f}" for r in ratio))
    R.gate(name, dict(ldj=t["ldj"][:rows]), r64, r32)
    assert torch.equal(t["dout"][:rows, d2 * d2:np_], c["dy2"])
    assert _zero(t["y2"][:rows, d2:]) and _zero(t["dx2"][:rows, d2:]) and _zero(t["dout"][:rows, np_:])
    for key in ("y2", "ldj", "dx2", "dout", "dscal"):
        assert (t[key][rows:] == 7.0).all(), f"{name}: {key} written beyond its rows"
    assert all(e <= limit for e in errs.values()), errs
    assert (ratio <= 4.0).all()


@pytest.mark.parametrize("name", ["x16_n16_r70", "x3_n03_r70"])
def test_expm_narrow_is_bit_stable_and_row_independent(name):
    c = R.make_expm_case(name)
    first, second = _run_expm(*_expm_inputs(c)), _run_expm(*_expm_inputs(c))
    assert first[0] == 0 and first[2] == 0
    assert all(torch.equal(first[1][k], second[1][k]) for k in first[1])
    for r in (3, 65):                                                    # a row of either 64-point block, alone
        code, alone, status = _run_expm(*_expm_inputs(c, [r]))
        assert code == 0 and status == 0
        assert all(torch.equal(alone[k][0], first[1][k][r]) for k in alone), f"{name}: row {r} alone differs"


def _run_expm_node(c, junk):
    rows, d2 = c["rows"], c["d2"]
    np_ = d2 * d2 + d2
    x2 = _in(c["x2"], True, junk)
    o = _in(torch.cat((c["raw"].reshape(rows, -1), c["b"]), 1), False, junk)
    cp = types.SimpleNamespace(**{n: torch.nn.Parameter(c["scal4"][i:i + 1].to(DEV)) for i, n in enumerate(("scale", "shift", "rescale", "reshift"))})
    _dirt((x2.shape[0], _r32(d2)), (x2.shape[0],))
    y2, ldj = T.expm_coupling(x2, o, cp, rows, d2)
    ups = [_up_grad(c["dy2"], y2, junk), _up_vec(c["dldj"], ldj, junk)]
    _dirt(tuple(x2.shape), tuple(o.shape))
    torch.autograd.backward([y2, ldj], ups)
    y2, ldj = y2.detach(), ldj.detach()
    hip = dict(y2=y2[:rows, :d2], ldj=ldj[:rows], dx2=x2.grad[:rows, :d2], draw=o.grad[:rows, :d2 * d2], db=o.grad[:rows, d2 * d2:np_],
               ds4=torch.cat([getattr(cp, n).grad for n in ("scale", "shift", "rescale", "reshift")]))
    return hip, _pads(rows, y2=(y2, d2), ldj=(ldj, 0), dx2=(x2.grad, d2), do=(o.grad, np_))


def test_expm_coupling_node_matches_fp64():
    """One case through train_ops.expm_coupling: 70 rows in a 256-row panel with junk in the pad rows, x2 in a wider panel; the four scalar
    gradients through _colsum."""
    name = "x15_n4_r70"
    c, r64, r32 = _case("expm", name)
    rows, d2 = c["rows"], c["d2"]
    hip, pads = _run_expm_node(c, 7.0)
    limit = R.expm_gate()
    errs = {k: R.rel(hip[k], r64[w].reshape(rows, -1), 0.0) for k, w in (("y2", "y"), ("dx2", "dx2"), ("draw", "draw"))}
    v, v64, v32 = hip["ds4"].double().cpu(), r64["dscal"], r32["dscal"].double()
    ratio = (v - v64).abs() / torch.maximum((v32 - v64).abs(), 4 * 2.0 ** -24 * r64["terms"])
    print(f"{name} (node): gate {limit:.1e}  " + "  ".join(f"{k} {e:.1e}" for k, e in errs.items()) + "  ds4 |v - v64| / E "
          + " ".join(f"{float(r):.2f}" for r in ratio))
    R.gate(name + " (node)", dict(ldj=hip["ldj"]), r64, r32)
    _assert_zero(name, pads)
    assert torch.equal(hip["db"].cpu(), c["dy2"])
    assert all(e <= limit for e in errs.values()), errs
    assert (ratio <= 4.0).all()
    again, _ = _run_expm_node(c, 0.0)                                    # bit for bit, whatever the pad rows hold
    assert all(torch.equal(hip[k], again[k]) for k in hip)


def test_expm_bwd_refuses_d2_17():
    d2, rows = 17, 2
    raw, x2, b, dy2, dldj, scal4 = R.make_case(d2, 0.3, rows, seed=1)
    o, xp, dyp = _panels(raw, x2, b, dy2)
    code, t, status = _run_expm(o, xp, dyp, dldj.to(DEV), scal4.to(DEV), d2, rows, forward=False)
    assert code == FC_ERR_INVALID and status == 0
    assert (t["dx2"] == 7.0).all() and (t["dout"] == 7.0).all() and (t["dscal"] == 7.0).all()        # nothing was launched


def test_expm_norm_beyond_32_raises_from_the_status_word():
    """Every row at |W|_inf > 32 (asserted on the CPU): more squarings than the 64 stored states.  An error return, and the last launch of
    this test."""
    c = R.make_expm_case("bound")
    rows, d2 = c["rows"], c["d2"]
    x2 = _in(c["x2"], False, 0.0, grad=False)
    o = _in(torch.cat((c["raw"].reshape(rows, -1), c["b"]), 1), False, 0.0, grad=False)
    with pytest.raises(RuntimeError, match=r"a matrix norm exceeds 2\^5"):
        T.ExpmCouplingFn.apply(x2, o, c["scal4"].to(DEV), rows, d2)


# ================================================================ column sums (csrc/train_wgrad.hip), called directly
# rows, cols, lda, base offset in floats, accumulate, splits (colsum_chunks: rows / 128 within [1, 256])
COLSUM_CASES = [
    (1, 4, 32, 0, 0, 1),
    (127, 35, 64, 0, 1, 1),                 # cols % 4 != 0: the scalar fallback at the tail
    (256, 300, 320, 0, 0, 2),
    (1000, 35, 64, 0, 0, 7),
    (1000, 300, 320, 0, 1, 7),
    (33000, 300, 320, 0, 0, 256),
    (33000, 4, 32, 0, 1, 256),
    (1000, 35, 37, 0, 1, 7),                # lda % 4 != 0: every lane on the scalar fallback
    (256, 300, 320, 1, 0, 2),               # base pointer one float beyond a 16-byte boundary: the same
    (127, 4, 4, 1, 1, 1),
]
SPARE_ROWS = 7


def _colsum(a, lda, cols, rows, out0, accumulate):
    L = engine.lib()
    out = out0.clone()
    nb = L.fc_train_colsum_ws_bytes(cols, rows)
    ws = T._ws(nb, torch.device(DEV))
    L.fc_train_colsum_f32(engine._ptr(a), lda, cols, rows, engine._ptr(out), accumulate, engine._ptr(ws), nb, engine._stream())
    return out.cpu()


def _offset_copy(a2d, offset):
    """The same [n, lda] values at a base pointer `offset` floats beyond an allocation's (16-byte aligned) start."""
    buf = torch.empty(a2d.numel() + 4, device=DEV)
    view = buf[offset:offset + a2d.numel()].view(a2d.shape)
    view.copy_(a2d)
    assert view.data_ptr() % 16 == 4 * offset
    return view


@pytest.mark.parametrize("rows,cols,lda,offset,accumulate,splits", COLSUM_CASES)
def test_colsum_matches_fp64(rows, cols, lda, offset, accumulate, splits):
    assert engine.lib().fc_train_colsum_ws_bytes(cols, rows) == splits * _r32(cols) * 4 + 256
    g = torch.Generator().manual_seed(rows + cols + lda)
    a = torch.randn(rows + SPARE_ROWS, lda, generator=g) + 0.3 * torch.randn(lda, generator=g)
    a[rows:] = 1e3                                                       # rows beyond `rows`, and the columns beyond `cols`, are someone else's
    clean = a.clone()
    clean[rows:] = 0
    clean[:, cols:] = 0
    out0 = torch.randn(cols + 3, generator=g) if accumulate else torch.full((cols + 3,), 7.0)
    base = out0[:cols] if accumulate else torch.zeros(cols)
    r64 = dict(sum=base.double() + a[:rows, :cols].double().sum(0))
    r32 = dict(sum=base + a[:rows, :cols].sum(0))
    dev_a, dev_clean = _offset_copy(a, offset), _offset_copy(clean, offset)
    first = _colsum(dev_a, lda, cols, rows, out0.to(DEV), accumulate)
    R.gate(f"colsum rows {rows} cols {cols} lda {lda} offset {offset} accumulate {accumulate}", dict(sum=first[:cols]), r64, r32)
    assert torch.equal(first[cols:], out0[cols:])
    assert torch.equal(first, _colsum(dev_a, lda, cols, rows, out0.to(DEV), accumulate))
    assert torch.equal(first, _colsum(dev_clean, lda, cols, rows, out0.to(DEV), accumulate)), "rows or columns beyond the asked ones entered"


# ================================================================ the stand-alone activation passes (csrc/train_linear.hip), called directly
ACT_SEEDS = {"GELU": 0, "RELU": 1, "ELU": 2}


@pytest.mark.parametrize("act", ["GELU", "RELU", "ELU"])
def test_standalone_activation_passes_match_fp64(act):
    """fc_train_act_fwd_f32 over a whole [512, 160] panel; fc_train_act_bwd_f32 with rows = 300: rows beyond come out 0 whatever dy and u
    hold there (inf and NaN here).  (FC_TRAIN_FUSED_ACT is read at import and left alone: the entries are called directly.)"""
    L = engine.lib()
    rows_pad, ld, rows = 512, 160, 300
    g = torch.Generator().manual_seed(ACT_SEEDS[act])
    u, dy = 3 * torch.randn(rows_pad, ld, generator=g), torch.randn(rows_pad, ld, generator=g)
    assert (u != 0).all()
    refs = []
    for dtype in (torch.float64, torch.float32):
        x = u.detach().to(dtype).clone().requires_grad_(True)
        y = R.act_ref(x, act)
        (y[:rows] * dy[:rows].to(dtype)).sum().backward()
        refs.append(dict(y=y.detach(), du=x.grad[:rows]))
    ud = u.to(DEV)
    y = torch.full_like(ud, 7.0)
    L.fc_train_act_fwd_f32(engine._ptr(ud), engine._ptr(y), rows_pad, ld, T.ACT_IDS[act], engine._stream())
    ub, dyb = u.clone(), dy.clone()
    ub[rows:], dyb[rows:] = float("nan"), float("inf")
    ub[rows + 1], dyb[rows + 1] = float("inf"), float("nan")
    ub, dyb = ub.to(DEV), dyb.to(DEV)
    du = torch.full_like(ud, 7.0)
    L.fc_train_act_bwd_f32(engine._ptr(dyb), engine._ptr(ub), engine._ptr(du), rows_pad, rows, ld, T.ACT_IDS[act], engine._stream())
    R.gate(f"act {act}", dict(y=y, du=du[:rows]), *refs)
    assert _zero(du[rows:])
    du2 = torch.full_like(ud, 7.0)
    L.fc_train_act_bwd_f32(engine._ptr(dyb), engine._ptr(ub), engine._ptr(du2), rows_pad, rows, ld, T.ACT_IDS[act], engine._stream())
    assert torch.equal(du, du2)
