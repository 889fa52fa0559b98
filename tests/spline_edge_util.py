"""Edge-case inputs, parameter families and the ENVELOPE checker of the rational-quadratic spline tests (tests/test_spline_edges_host.py on the
CPU, tests/test_gpu_spline_edges.py on the kernels of csrc/spline.h).

Why an envelope.  Near the knots of floor-width bins log|det| is ill-conditioned in x (a bin 0.006 wide between knot derivatives 0.005 and 4.8
moves it by about a nat per fp32 ulp of x; the oracle's own fp32 run is 0.3 nats from its fp64 run there), so a point-wise tolerance is either
useless or flaky.  What IS well conditioned is a backward-error statement: the value under test must lie inside [min, max] of the fp64 oracle
over the shifts |s| <= 8 R 2^-25 of x (R in units of 2^-22, the fp32 spacing at 3.0; grid x + i 2^-25).  y and log|det| are continuous across interior
knots (the spline is C1), so the envelope also makes the check independent of the side of a knot an fp32 evaluation lands on.  Elements outside
[-3, 3] are not shifted, shifts of inside elements are clamped to [-3, 3] (the fp32 inside / outside decision is exact), and outside elements
must come back as y == x bit for bit with log|det| == 0.

Tolerance rule (the project's own: tests/test_gpu_train.py, 3 x fp32 oracle + a floor).  Per family and quantity
    tol = 3 x (residual of oracle.flow_oracle.rq_spline in fp32 against the same envelope) + floor,
floors = the element gates of tests/test_gpu_ops.py::test_spline_golden_forward_and_inverse (2e-5 on y, 2e-4 on log|det|).  The fp32 oracle's
residual is computed here, on the CPU, never from a kernel.  No family's log|det| tolerance may exceed LAD_TOL_CAP = 5e-3
(tests/test_spline_edges_host.py asserts it).

The envelope is the fp64 oracle's range over the INTERVAL, sampled on that grid and at every fp64 knot inside it (see envelope()).

R = 4: the smallest of {1, 2, 4, 8} from which on no family's fp32-oracle log|det| residual shrinks by more than a tenth of the floor any more
(an fp32 cumulative sum puts a knot up to ~4 units of 2^-22 from its fp64 place; at R = 2 "one wide bin" still shows 1e-2 and "lively" 0.49 at
K = 16); what is left is parameter and evaluation rounding, not knot position.  Measured on the CPU, forward, worst element
(tests/test_spline_edges_host.py prints this table and pins R):

     K  family                              y at R = 4   log|det| at R = 1 / 2 / 4 / 8
     4  uniform                             0.0e+00      5.5e-08 / 5.5e-08 / 5.5e-08 / 5.5e-08
     4  lively                              9.3e-07      4.9e-05 / 4.7e-05 / 4.3e-05 / 3.5e-05
     4  one wide bin                        2.4e-07      9.6e-02 / 1.5e-02 / 8.5e-05 / 8.4e-05
     4  ramps + softplus switch             2.6e-08      1.8e-03 / 8.4e-05 / 8.4e-05 / 8.4e-05
     4  floor bins at both ends             5.6e-07      1.0e-03 / 1.6e-04 / 1.6e-07 / 1.6e-07
     4  flushed exponentials                3.8e-07      9.0e-04 / 1.3e-04 / 7.4e-06 / 6.0e-06
     4  flat bin between knots beyond 10    2.4e-07      5.7e-06 / 1.6e-07 / 1.6e-07 / 1.6e-07
     8  uniform                             0.0e+00      5.5e-08 / 5.5e-08 / 5.5e-08 / 5.5e-08
     8  lively                              6.4e-07      4.1e-04 / 2.3e-04 / 9.7e-06 / 3.5e-07
     8  one wide bin                        3.8e-08      6.8e-02 / 1.0e-02 / 7.4e-05 / 7.4e-05
     8  ramps + softplus switch             5.7e-07      2.1e-03 / 1.6e-04 / 1.5e-04 / 1.5e-04
     8  floor bins at both ends             1.2e-07      1.6e-07 / 1.6e-07 / 1.6e-07 / 1.6e-07
     8  flushed exponentials                3.0e-07      1.6e-04 / 3.2e-05 / 3.2e-05 / 3.2e-05
     8  flat bin between knots beyond 10    6.4e-07      9.1e-05 / 4.2e-05 / 1.0e-05 / 9.5e-06
    16  uniform                             0.0e+00      5.5e-08 / 5.5e-08 / 5.5e-08 / 5.5e-08
    16  lively                              5.5e-07      6.9e-01 / 4.9e-01 / 4.2e-05 / 2.8e-05
    16  one wide bin                        2.6e-07      1.7e-01 / 8.7e-05 / 8.7e-05 / 8.6e-05
    16  ramps + softplus switch             7.6e-07      3.9e-03 / 8.1e-04 / 1.4e-04 / 1.4e-04
    16  floor bins at both ends             8.5e-07      2.7e-03 / 1.7e-03 / 1.6e-07 / 1.6e-07
    16  flushed exponentials                2.3e-07      1.1e-04 / 1.1e-04 / 1.1e-04 / 1.1e-04
    16  flat bin between knots beyond 10    2.0e-07      5.5e-05 / 1.7e-05 / 1.6e-05 / 1.5e-05

(The oracle's fp32 run places its knots this well because ATen's CPU cumsum accumulates float in double (and its softmax comes out within an ulp).  A pure-fp32 evaluation that
adds the terms one by one is 8.6 units off on "flat bin between knots beyond 10" at K = 16 and 6 .. 10 units off on random lively parameters:
tests/test_gpu_spline_edges.py records what that did to the kernels at K = 16, which now add in blocks of four there.)

The worst forward tolerance is therefore 3 x 1.5e-4 + 2e-4 = 6.5e-4 on log|det| and 3 x 9.3e-7 + 2e-5 = 2.3e-5 on y.  Inverse direction: see case().
"""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import flow_oracle as O

BOUND = 3.0
R = 4                               # envelope radius in units of 2^-22 (see above)
STEP = 2.0 ** -25                   # grid step of the envelope: an eighth of the fp32 spacing at 3.0
FLOOR_Y, FLOOR_LAD = 2e-5, 2e-4     # tests/test_gpu_ops.py::test_spline_golden_forward_and_inverse
FLOOR_RT_Y, FLOOR_RT_LAD = 5e-5, 5e-4     # the same test's round-trip gates
LAD_TOL_CAP = 5e-3
BINS = (4, 8, 16)


def _f32(t):
    """values every party sees alike: rounded to fp32, held in fp64"""
    return torch.as_tensor(t, dtype=torch.float64).float().double()


def _next32(v, towards):
    return float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(towards, dtype=torch.float32)))


@functools.lru_cache(maxsize=None)
def families(K, inverse=False):
    """[(name, fp64 vector [K widths | K heights | K+1 derivative logits] of fp32-representable values)].  Seven families: coprime to the 5 dims
    of a K = 8 parameter tile and to the lane halves, so the mixed run of the fused tests puts every family on every tile position."""
    g = torch.Generator().manual_seed(1000 + K)
    zeros = lambda n: torch.zeros(n, dtype=torch.float64)
    cyc = lambda vals, n: torch.tensor([vals[i % len(vals)] for i in range(n)], dtype=torch.float64)
    out = [("uniform", torch.cat((zeros(K), zeros(K), zeros(K + 1))))]
    out.append(("lively", 3.0 * torch.randn(3 * K + 1, generator=g, dtype=torch.float64)))
    w, h = zeros(K), zeros(K)
    w[K // 4], h[(3 * K) // 4] = 30.0, 30.0                                 # one wide bin, one tall bin: every other at its floor
    out.append(("one wide bin", torch.cat((w, h, torch.randn(K + 1, generator=g, dtype=torch.float64)))))
    switch = [20.0, _next32(20.0, math.inf), _next32(20.0, -math.inf), 25.0, -30.0, -5.0, 40.0, 0.0, 7.0]
    if inverse:
        # the inverse's own version (a family that needs more than LAD_TOL_CAP is replaced): with knot derivatives of 40 and 1e-3 beside bins
        # 0.006 tall the fp32 oracle's inverse is 1e-2 off at K = 8 even on well-conditioned elements; the extremes come in to 12 and -8
        switch = [20.0, _next32(20.0, math.inf), _next32(20.0, -math.inf), 12.0, -8.0, -5.0, 12.0, 0.0, 7.0]
    out.append(("ramps + softplus switch", torch.cat((torch.linspace(-12, 12, K, dtype=torch.float64), torch.linspace(12, -12, K, dtype=torch.float64),
                                                     cyc(switch, K + 1)))))
    w = zeros(K)
    w[0] = w[K - 1] = -40.0
    out.append(("floor bins at both ends", torch.cat((w, w.clone(), cyc([-20.0, 3.0, -3.0, 10.0, -10.0, 0.0, 1.0, -20.0, 0.0], K + 1)))))
    # Softmax logit differences of 88 .. 150 (beyond 88 an fp32 exp gives a denormal and v_exp zero, beyond 104 both give zero): every bin but one
    # wide and two tall ones at its floor.  The wide bin is tall as well (2.98 of the 6), with both its knots' derivative logits just beyond 10:
    # the one place where softplus(v) - v = e^-10 moves the inverse by more than the gates.
    j, j2 = K // 2, K // 2 - 2
    w, h = cyc([-60.0, -74.0, -80.0, -120.0, -65.0, -58.0, -90.0, -100.0], K), cyc([0.0, 16.5, 30.0, -30.0, 15.0, 10.0, 31.5, 17.0], K)
    w[j], h[j], h[j2] = 30.0, 120.0, 120.0
    d = cyc([-90.0, 0.5, -104.0, 1e-30, -1e-3, 2.0, 1.0, -0.5, 0.0], K + 1)
    d[j - 1] = d[j] = 10.0001
    out.append(("flushed exponentials", torch.cat((w, h, d))))
    # One bin 5.5 wide and 1.65 tall (slope 0.3; 0.018 in its middle) between knots whose derivative logits lie just beyond and just below 10 (y depends on their ratio), every other bin of
    # moderate slope, all derivative logits distinct.  The one place where softplus(v) - v = e^-10 shows: forward it moves y by 7e-6 at most,
    # below the floors, but the inverse divides that by the slope.  Distinct logits also show a select that goes one slot wrong at every knot.
    j = K // 2
    share = lambda size: (size / 6.0 - 1e-3) / (1 - 1e-3 * K)
    logit = lambda s_: math.log(s_ / (1 - s_) * (K - 1))
    w, h, d = zeros(K), zeros(K), torch.linspace(-2, 2, K + 1, dtype=torch.float64)
    w[j], h[j] = logit(share(5.5)), logit(share(1.65))
    d[j - 1], d[j] = 10.0001, 9.9999
    out.append(("flat bin between knots beyond 10", torch.cat((w, h, d))))
    return tuple((n, _f32(p)) for n, p in out)


def knots64(p, K):
    """fp64 knots (widths, heights) of parameter vectors p [..., 3K+1]: -3, -3 + 6 cumsum(1e-3 + (1 - 1e-3 K) softmax), 3"""
    out = []
    for u in (p[..., :K], p[..., K:2 * K]):
        c = torch.cumsum(1e-3 + (1 - 1e-3 * K) * torch.softmax(u.double(), -1), -1)
        c = torch.cat((torch.zeros_like(c[..., :1]), c), -1) * 2 * BOUND - BOUND
        c[..., 0], c[..., -1] = -BOUND, BOUND
        out.append(c)
    return out


def edge_inputs(p, K, inverse):
    """fp32 inputs of one family: every fp64 knot of the searched axis rounded to fp32 with its +-1..8 ulp neighbours, +-3 and the next value
    outward, 3.000001 and 3.0000012 (inside the +1e-6 search margin, outside the domain), +-3.5, 0.0, -0.0, 1e-30, every bin midpoint."""
    kn = knots64(p, K)[1 if inverse else 0]
    vals = []
    for k in kn.float():
        up = dn = k
        vals.append(k)
        for _ in range(8):
            up, dn = torch.nextafter(up, torch.tensor(math.inf)), torch.nextafter(dn, torch.tensor(-math.inf))
            vals += [up, dn]
    x = torch.stack(vals)
    extra = torch.tensor([-3.0, 3.0, _next32(3.0, math.inf), _next32(-3.0, -math.inf), 3.000001, 3.0000012, 3.5, -3.5, 0.0, -0.0, 1e-30], dtype=torch.float32)
    mid = ((kn[1:] + kn[:-1]) / 2).float()
    return torch.cat((x, extra, mid))


def oracle(x, p, K, inverse, dtype):
    """oracle.flow_oracle.rq_spline on x [...] with parameters p [..., 3K+1] (broadcast against x) in `dtype`; returns fp64"""
    p = p.to(dtype).expand(*x.shape, 3 * K + 1)
    y, lad = O.rq_spline(x.to(dtype), p[..., :K], p[..., K:2 * K], p[..., 2 * K:], inverse=inverse)
    return y.double(), lad.double()


def envelope(x32, p64, K, inverse=False, r=R):
    """(y_lo, y_hi, lad_lo, lad_hi) of the fp64 oracle over the interval |shift| <= 8 r 2^-25 around x: sampled at x + i 2^-25, |i| <= 8 r, and at
    every fp64 knot of the searched axis inside the interval (log|det| has its kinks there, and between floor-width bins it moves by 1e-3 within a
    sixteenth of an ulp: the grid alone would miss the extremum the fp32 evaluation hits when it lands ON the knot).  x32 [n] fp32, p64 [n, 3K+1]
    or [3K+1]."""
    assert x32.dtype == torch.float32
    x = x32.double()
    p64 = p64.double().expand(x.numel(), 3 * K + 1)
    inside = (x >= -BOUND) & (x <= BOUND)
    i = torch.arange(-8 * r, 8 * r + 1, dtype=torch.float64)[:, None] * STEP
    xs = torch.where(inside[None], (x[None] + i).clamp(-BOUND, BOUND), x[None].expand(i.shape[0], -1))
    kn = knots64(p64, K)[1 if inverse else 0].t()                                              # [K+1, n]
    near = inside[None] & ((kn - x[None]).abs() <= 8 * r * STEP)
    xs = torch.cat((xs, torch.where(near, kn, x[None].expand(K + 1, -1))))
    y, lad = oracle(xs, p64, K, inverse, torch.float64)
    return y.min(0)[0], y.max(0)[0], lad.min(0)[0], lad.max(0)[0]


def residuals(x32, p64, K, y, lad, inverse=False, r=R, env=None, exact_outside=True):
    """Per element, how far y and lad lie outside the envelope (0 inside it).  Elements outside [-3, 3] must be y == x bit for bit and
    lad == 0; one that is not, and any NaN, counts as an infinite residual.  (exact_outside = False, for a y that went through another
    layer's arithmetic after the spline: an outside element's |y - x| is its residual like any other; lad may then be None.)"""
    lo_y, hi_y, lo_l, hi_l = env if env is not None else envelope(x32, p64, K, inverse, r)
    y = y.detach().cpu()
    lad = None if lad is None else lad.detach().cpu()
    x = x32.double()
    outside = ~((x >= -BOUND) & (x <= BOUND))
    res = []
    for v, lo, hi in ((y.double(), lo_y, hi_y),) + (() if lad is None else ((lad.double(), lo_l, hi_l),)):
        d = torch.maximum(lo - v, v - hi).clamp_min(0.0)
        res.append(torch.where(torch.isnan(v), torch.full_like(d, math.inf), d))
    if not exact_outside:
        return tuple(res)
    if y.dtype == torch.float32:
        exact = (y.view(torch.int32) == x32.view(torch.int32)) & (lad == 0)
    else:
        exact = (y == x) & (lad == 0)
    bad = outside & ~exact
    return tuple(torch.where(bad, torch.full_like(d, math.inf), d) for d in res)


def per_family(values, fam, n_fam):
    """worst element of every family"""
    return [float(values[fam == f].max()) for f in range(n_fam)]


def gates(ry, rl, fam, n_fam, floor_y=FLOOR_Y, floor_lad=FLOOR_LAD):
    """the tolerance rule on the fp32 oracle's residuals ry, rl [n]: per family 3 x worst + floor"""
    ref_y, ref_lad = per_family(ry, fam, n_fam), per_family(rl, fam, n_fam)
    return dict(ref_y=ref_y, ref_lad=ref_lad, tol_y=[3.0 * v + floor_y for v in ref_y], tol_lad=[3.0 * v + floor_lad for v in ref_lad])


U32 = 2.0 ** -24                     # fp32 unit roundoff
KNOT_ERR = 2.0 ** -20                # 4 units of 2^-22: how far an fp32 knot may sit from its fp64 place (= R)


def inverse_error_estimate(y32, p64, K, env):
    """What fp32 can be asked of the reference's INVERSE formula at each element, estimated in fp64 from the formula itself (never from a
    kernel, nor from one fp32 run's rounding luck): returns (ex, el), how far the recovered point and log|det| come to lie OUTSIDE the envelope
    `env` of the check (which already forgives what a shift of y explains) when
      * the three cancelling differences of the quadratic (qa, qb and the discriminant qb^2 - 4 qa qc) are disturbed by 2 roundings of their
        larger term,
      * the bin's height is disturbed by KNOT_ERR (one knot off by what R allows), and
      * y lies within KNOT_ERR above a height knot and is evaluated in the bin BELOW it instead, root beyond 1, as an fp32 run whose knot sits a
        little higher does.
    An element whose estimate exceeds a quarter of the floor (FLOOR_Y, FLOOR_LAD; the disturbances are taken one at a time) is ill-conditioned for that quantity: case() leaves it out of the
    tolerance AND out of the gate; everything else of every family is gated."""
    y, p = y32.double(), p64.double().expand(y32.numel(), 3 * K + 1)
    cw, ch = knots64(p, K)
    loc = ch.clone()
    loc[:, -1] += 1e-6
    b0 = ((y[:, None] >= loc).sum(-1) - 1).clamp(0, K - 1)
    g = lambda t, i: t.gather(-1, i[:, None])[:, 0]
    d = 1e-3 + F.softplus(torch.cat((torch.full_like(p[:, :1], math.log(math.exp((1 - 1e-3) - 1))), p[:, 2 * K:]), -1))

    def solve(b, dh=0.0, sd=0, sa=0, sb=0):
        d0, d1 = g(d, b), g(d, b + 1)
        in_cw, in_w, in_ch, in_h = g(cw, b), g(cw, b + 1) - g(cw, b), g(ch, b), g(ch, b + 1) - g(ch, b) + dh
        delta, dy = in_h / in_w, y - in_ch
        t3 = d0 + d1 - 2 * delta
        qa = dy * t3 + in_h * (delta - d0) + sa * U32 * ((dy * t3).abs() + (in_h * (delta - d0)).abs())
        qb = in_h * d0 - dy * t3 + sb * U32 * ((in_h * d0).abs() + (dy * t3).abs())
        qc = -delta * dy
        disc = (qb * qb - 4 * qa * qc + sd * U32 * (qb * qb + (4 * qa * qc).abs())).clamp_min(0.0)
        root = (2 * qc) / (-qb - disc.sqrt())
        tt = root * (1 - root)
        lad = -(torch.log(delta ** 2 * (d1 * root ** 2 + 2 * delta * tt + d0 * (1 - root) ** 2)) - 2 * torch.log(delta + t3 * tt))
        return root * in_w + in_cw, lad
    ex, el = torch.zeros_like(y), torch.zeros_like(y)
    outside = lambda v, lo, hi: torch.nan_to_num(torch.maximum(lo - v, v - hi).clamp_min(0.0), nan=math.inf)
    below = (b0 > 0) & (y - g(ch, b0) <= KNOT_ERR)
    for v in (dict(dh=KNOT_ERR), dict(dh=-KNOT_ERR), dict(sd=2), dict(sd=-2), dict(sa=2), dict(sa=-2), dict(sb=2), dict(sb=-2), None):
        x, lad = solve(b0, **v) if v is not None else solve((b0 - 1).clamp_min(0))
        dx, dl = outside(x, env[0], env[1]), outside(lad, env[2], env[3])
        if v is None:
            dx, dl = dx.masked_fill(~below, 0.0), dl.masked_fill(~below, 0.0)
        ex, el = torch.maximum(ex, dx), torch.maximum(el, dl)
    inside = (y >= -BOUND) & (y <= BOUND)
    return ex.masked_fill(~inside, 0.0), el.masked_fill(~inside, 0.0)


@functools.lru_cache(maxsize=None)
def case(K, inverse=False, r=R):
    """Everything the tests share about one (K, direction), made once and never modified: inputs x [n] (fp32), parameters p [n, 3K+1] (fp64, one
    family per element: fam [n]), the envelope, the fp32 oracle's results and residuals, and the tolerances per family:
    c["direct"].  Every family is gated in both directions.  Inverse: the reference's quadratic-root formula loses its digits in fp32 on SINGLE
    elements (a discriminant that is a difference of numbers of order one in steep or flat bins; y within a knot's error of a height knot:
    there the fp32 oracle returns points 1e-4 beyond +3, roots 6 % of a bin off, log|det| nats away or NaN).  Those elements, found by
    inverse_error_estimate in fp64, are left out element by element and per quantity (c["ill_y"], c["ill_lad"]); tests/test_spline_edges_host.py
    pins how many there may be."""
    fams = families(K, inverse)
    xs, ps, fs = [], [], []
    for f, (_, p) in enumerate(fams):
        x = edge_inputs(p, K, inverse)
        xs.append(x)
        ps.append(p[None].expand(x.numel(), -1))
        fs.append(torch.full((x.numel(),), f, dtype=torch.long))
    x, p, fam = torch.cat(xs), torch.cat(ps).contiguous(), torch.cat(fs)
    return _tables(dict(K=K, inverse=inverse, names=[n for n, _ in fams], x=x, p=p, fam=fam), r)


def _tables(c, r=R):
    """envelope, fp32 oracle, its residuals and the tolerances for the elements c["x"], c["p"], c["fam"]"""
    x, p, fam, K, inverse = c["x"], c["p"], c["fam"], c["K"], c["inverse"]
    with torch.no_grad():
        c["env"] = envelope(x, p, K, inverse, r)
        c["y32"], c["lad32"] = (t.float() for t in oracle(x, p, K, inverse, torch.float32))
        ry, rl = residuals(x, p, K, c["y32"], c["lad32"], inverse, env=c["env"])
        if inverse:
            ex, el = inverse_error_estimate(x, p, K, c["env"])
            c["ill_y"], c["ill_lad"] = ex > FLOOR_Y / 4, el > FLOOR_LAD / 4          # (four disturbances, taken one at a time: a quarter each)
        else:
            c["ill_y"] = c["ill_lad"] = torch.zeros_like(fam, dtype=torch.bool)
        c["direct"] = gates(ry.masked_fill(c["ill_y"], 0.0), rl.masked_fill(c["ill_lad"], 0.0), fam, len(c["names"]))
    return c


@functools.lru_cache(maxsize=None)
def flow_inputs(K, B=2, N=300, seed=7):
    """Inputs of the crafted-flow tests (tests/test_gpu_spline_edges.py): per family f a table X[f] [B, N] of layer-0 spline inputs -- row r of
    scene 0 carries edge input r, scene 1 carries the list reversed, the rows left over carry random points inside (-2.9, 2.9) -- and the element
    tables of case() over all F B N of them (forward; c["fy64"], c["flad64"]: the fp64 oracle at x itself)."""
    fams = families(K)
    g = torch.Generator().manual_seed(seed + K)
    X = (torch.rand(len(fams), B, N, generator=g) * 5.8 - 2.9).float()
    for f, (_, p) in enumerate(fams):
        x = edge_inputs(p, K, False)
        n = min(x.numel(), N)
        X[f, 0, :n] = x[:n]
        for b in range(1, B):
            X[f, b, :n] = x.flip(0)[:n]
        assert B >= 2 and 2 * N >= x.numel()
    p = torch.stack([p for _, p in fams])[:, None].expand(-1, B * N, -1).reshape(-1, 3 * K + 1).contiguous()
    fam = torch.arange(len(fams))[:, None].expand(-1, B * N).reshape(-1)
    c = _tables(dict(K=K, inverse=False, names=[n for n, _ in fams], x=X.reshape(-1).clone(), p=p, fam=fam, X=X))
    assert max(c["direct"]["tol_lad"]) <= LAD_TOL_CAP
    c["fy64"], c["flad64"] = oracle(c["x"], c["p"], K, False, torch.float64)
    return c


@functools.lru_cache(maxsize=None)
def round_trip(K):
    """The round trip forward(inverse(y)) of the inverse case: which elements it is asked of, and its tolerances.  Left out, by fp64 criteria:
    |y| >= 2.999 (tests/test_gpu_ops.py's golden round trip: a recovered point may round across +-3), the inverse's ill-conditioned elements
    (case()), and elements where ROUNDING the recovered point to fp32 moves the forward result by itself: the fp64 forward envelope of radius
    1 around the fp64 recovered point is wider than a quarter of the round-trip floors (log|det| moves by a nat per ulp in floor-width bins).
    Tolerances: 3 x the fp32 oracle's own round trip on the kept elements + the golden round-trip gates."""
    c = case(K, True)
    with torch.no_grad():
        x64, _ = oracle(c["x"], c["p"], K, True, torch.float64)
        ylo, yhi, llo, lhi = envelope(torch.nan_to_num(x64).float(), c["p"], K, False, r=1)
        keep = (c["x"].abs() < 2.999) & ~c["ill_y"] & ~c["ill_lad"] & ~torch.isnan(x64) & (yhi - ylo <= FLOOR_RT_Y / 4) & (lhi - llo <= FLOOR_RT_LAD / 4)
        xo, lo = (t.float() for t in oracle(c["x"], c["p"], K, True, torch.float32))
        y2o, l2o = oracle(xo, c["p"], K, False, torch.float32)
    err = lambda v: torch.nan_to_num(v.double().abs(), nan=math.inf).masked_fill(~keep, 0.0)
    return dict(keep=keep, err=err, gates=gates(err(y2o - c["x"]), err(l2o + lo), c["fam"], len(c["names"]), FLOOR_RT_Y, FLOOR_RT_LAD))


def report(label, names, fam, ry, rl, g):
    """One log line per family (worst y and log|det| residual of the values under test, the fp32 oracle's, the tolerance) and the verdict: the
    names of the families that miss a tolerance (empty = pass)."""
    failed = []
    for f, name in enumerate(names):
        wy, wl = float(ry[fam == f].max()), float(rl[fam == f].max())
        ok = wy <= g["tol_y"][f] and wl <= g["tol_lad"][f]
        print(f"{label} | {name}: y residual {wy:.2e} (fp32 oracle {g['ref_y'][f]:.2e}, tol {g['tol_y'][f]:.2e})  log|det| residual {wl:.2e} "
              f"(fp32 oracle {g['ref_lad'][f]:.2e}, tol {g['tol_lad'][f]:.2e})" + ("" if ok else "   <-- MISSES"))
        if not ok:
            failed.append(name)
    return failed


def check(label, c, y, lad):
    """the check of a result of c's direction: every family, every element but the ill-conditioned ones of the inverse (see case())"""
    ry, rl = residuals(c["x"], c["p"], c["K"], y, lad, c["inverse"], env=c["env"])
    return report(label, c["names"], c["fam"], ry.masked_fill(c["ill_y"], 0.0), rl.masked_fill(c["ill_lad"], 0.0), c["direct"])
