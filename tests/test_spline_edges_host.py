"""The envelope checker of tests/spline_edge_util.py must be able to fail: the fp32 oracle passes it on every family at K = 4, 8, 16, forward and
inverse, and seven planted faults -- small variants of the spline arithmetic, written out below in fp32 -- each miss it on at least one family
with the same tolerances.  Runs on the CPU."""
import pytest
import torch
import torch.nn.functional as F

import spline_edge_util as SU

FAULTS = {
    1: "pad logit 0 instead of -1e-3",
    2: "derivative logit i instead of i - 1 for the lower knot",
    3: "dead logit K used for the last bin's upper knot",
    4: "no +1e-6 on the last knot: x = 3 falls off the end",
    5: "x = +-3 treated as outside",
    6: "bin index off by one for x exactly on a knot, lower edge taken from the other side",
    7: "softplus switch at 20 replaced by the linear branch from 10",
}


def spline32(x, p, K, inverse=False, fault=0):
    """The spline of csrc/spline.h in plain fp32 tensor arithmetic, x [n], p [n, 3K+1]; fault = a key of FAULTS, 0 = none."""
    x, p = x.float(), p.float()
    uw, uh, ud = p[:, :K], p[:, K:2 * K], p[:, 2 * K:]
    inside = ((x > -3.0) & (x < 3.0)) if fault == 5 else ((x >= -3.0) & (x <= 3.0))
    xc = torch.where(inside, x, torch.zeros_like(x))

    def knots(u):
        c = torch.cumsum(1e-3 + (1 - 1e-3 * K) * torch.softmax(u, -1), -1)
        c = 6.0 * F.pad(c, (1, 0)) - 3.0
        c[:, 0], c[:, -1] = -3.0, 3.0
        return c
    cw, ch = knots(uw), knots(uh)
    loc = (ch if inverse else cw).clone()
    if fault != 4:
        loc[:, -1] += 1e-6
    b = (xc[:, None] >= loc).sum(-1) - 1
    b = torch.where(b >= K, torch.zeros_like(b), b)                 # fault 4: no bin matches, the selects keep what they started with (bin 0)
    b_edge = b
    if fault == 6:
        on_knot = (xc[:, None] == loc[:, 1:K]).any(-1)
        b = b - on_knot.long()                                      # the bin below the knot for everything but the lower edge
    g = lambda t, i: t.gather(-1, i[:, None])[:, 0]
    in_cw, in_ch = (g(cw, b_edge), g(ch, b)) if not inverse else (g(cw, b), g(ch, b_edge))
    in_w, in_h = g(cw[:, 1:] - cw[:, :-1], b), g(ch[:, 1:] - ch[:, :-1], b)
    pad = torch.full_like(ud[:, :1], 0.0 if fault == 1 else -1e-3)
    lower = torch.cat((pad, ud[:, 1:K] if fault == 2 else ud[:, :K - 1]), -1)                   # logit of knot i = ud[i - 1]
    upper = torch.cat((ud[:, :K - 1], ud[:, K:K + 1]), -1) if fault == 3 else ud[:, :K]         # logit of knot i + 1 = ud[i]
    softplus = (lambda v: torch.where(v > 10.0, v, torch.log1p(torch.exp(v.clamp_max(10.0))))) if fault == 7 else F.softplus
    d0, d1 = 1e-3 + softplus(g(lower, b)), 1e-3 + softplus(g(upper, b))
    delta = in_h / in_w
    if inverse:
        dy = xc - in_ch
        t3 = d0 + d1 - 2 * delta
        qa, qb, qc = dy * t3 + in_h * (delta - d0), in_h * d0 - dy * t3, -delta * dy
        th = ((2 * qc) / (-qb - torch.sqrt((qb * qb - 4 * qa * qc).clamp_min(0.0)))).clamp_max(1.0)      # (both held at their bounds: csrc/spline.h)
        out = th * in_w + in_cw
    else:
        th = (xc - in_cw) / in_w
    tt = th * (1 - th)
    den = delta + (d0 + d1 - 2 * delta) * tt
    lad = torch.log(delta * delta * (d1 * th * th + 2 * delta * tt + d0 * (1 - th) * (1 - th))) - 2 * torch.log(den)
    if inverse:
        lad = -lad
    else:
        out = in_ch + in_h * (delta * th * th + d0 * tt) / den
    return torch.where(inside, out, x), torch.where(inside, lad, torch.zeros_like(lad))


def _name(K, inverse):
    return f"K {K} {'inverse' if inverse else 'forward'}"


# Upper bounds on the inverse's ill-conditioned elements (left out of the gate: spline_edge_util.case), (recovered point, log|det|) per K, and
# lower bounds on the elements the round trip is asked of per family: the gated set cannot shrink unnoticed.  Measured: 46 / 166 of 700,
# 37 / 367 of 1204, 46 / 709 of 2212; the edge inputs sit where the inverse is at its worst, and every family keeps elements in the gate.
ILL_AT_MOST = {4: (50, 175), 8: (42, 380), 16: (52, 730)}
ROUND_TRIP_AT_LEAST = {4: [58, 35, 15, 0, 22, 3, 32], 8: [130, 89, 18, 0, 78, 5, 52], 16: [274, 54, 65, 17, 162, 18, 47]}


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("K", SU.BINS)
def test_fp32_oracle_and_the_unfaulted_variant_pass(K, inverse):
    """... on every family, with no family's log|det| tolerance beyond LAD_TOL_CAP, in both directions"""
    c = SU.case(K, inverse)
    assert len(c["names"]) % 5 != 0 and len(c["names"]) % 2 != 0
    assert SU.check(f"fp32 oracle {_name(K, inverse)}", c, c["y32"], c["lad32"]) == []
    assert SU.check(f"plain fp32 variant {_name(K, inverse)}", c, *spline32(c["x"], c["p"], K, inverse)) == []
    assert max(c["direct"]["tol_lad"]) <= SU.LAD_TOL_CAP, f"a family's log|det| tolerance exceeds {SU.LAD_TOL_CAP}: replace it"
    n_y, n_lad = int(c["ill_y"].sum()), int(c["ill_lad"].sum())
    print(f"{_name(K, inverse)}: {c['x'].numel()} elements, left out as ill-conditioned: {n_y} recovered points, {n_lad} log|det|; per family "
          f"{[int((c['ill_lad'] & (c['fam'] == f)).sum()) for f in range(len(c['names']))]}")
    if not inverse:
        assert n_y == 0 and n_lad == 0
    else:
        assert n_y <= ILL_AT_MOST[K][0] and n_lad <= ILL_AT_MOST[K][1]
        assert all(int((~c["ill_lad"] & (c["fam"] == f)).sum()) >= 0.3 * int((c["fam"] == f).sum()) for f in range(len(c["names"])))


@pytest.mark.parametrize("K", SU.BINS)
def test_round_trip_keeps_its_elements_and_its_tolerances(K):
    c, rt = SU.case(K, True), SU.round_trip(K)
    kept = [int((rt["keep"] & (c["fam"] == f)).sum()) for f in range(len(c["names"]))]
    print(f"round trip K {K}: kept per family {kept}; tolerances y {rt['gates']['tol_y']} log|det| {rt['gates']['tol_lad']}")
    assert all(k >= m - 2 for k, m in zip(kept, ROUND_TRIP_AT_LEAST[K]))
    assert max(rt["gates"]["tol_lad"]) <= SU.LAD_TOL_CAP and max(rt["gates"]["tol_y"]) <= 10 * SU.FLOOR_RT_Y


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_faults_miss_the_checker(fault):
    caught = {}
    for K in SU.BINS:
        for inverse in (False, True):
            c = SU.case(K, inverse)
            failed = SU.check(f"fault {fault} {_name(K, inverse)}", c, *spline32(c["x"], c["p"], K, inverse, fault))
            if failed:
                caught[K, inverse] = failed
    print(f"fault {fault} ({FAULTS[fault]}): caught at {caught}")
    assert caught, f"fault {fault} ({FAULTS[fault]}) passes the checker everywhere"
    if fault != 7:
        assert all((K, False) in caught for K in SU.BINS), f"fault {fault}: not caught in the forward direction at every K: {caught}"


def test_envelope_radius_is_the_smallest_at_which_the_oracle_residual_stops_shrinking():
    """Prints the table of spline_edge_util's docstring and pins R: the smallest radius from which on no family's fp32-oracle log|det| residual
    shrinks by more than a tenth of the floor any more, at every K (forward: the direction the fused evaluators have)."""
    rows = {(K, r): SU.case(K, False, r)["direct"] for K in SU.BINS for r in (1, 2, 4, 8)}
    names = SU.case(8)["names"]
    for K in SU.BINS:
        for f, name in enumerate(names):
            print(f"K {K:2d} {name:34s} y {rows[K, SU.R]['ref_y'][f]:.1e}   log|det| " + " / ".join(f"{rows[K, r]['ref_lad'][f]:.1e}" for r in (1, 2, 4, 8)))
    settled = lambda r: all(rows[K, r]["ref_lad"][f] <= rows[K, 8]["ref_lad"][f] + 0.1 * SU.FLOOR_LAD for K in SU.BINS for f in range(len(names)))
    assert settled(SU.R) and not any(settled(r) for r in (1, 2, 4, 8) if r < SU.R)


def test_outside_elements_must_be_bit_exact():
    c = SU.case(8, False)
    out = (c["x"].abs() > 3).nonzero()[:, 0]
    assert out.numel() >= 5 * len(c["names"])
    for what in ("y", "lad"):
        y, lad = c["y32"].clone(), c["lad32"].clone()
        if what == "y":
            y[out[0]] = torch.nextafter(y[out[0]], torch.tensor(0.0))
        else:
            lad[out[1]] = 1e-30
        assert SU.check(f"outside element with {what} disturbed", c, y, lad) != []
