"""The embedder training operators one by one (csrc/train_edge.hip through train_ops.BatchNormMaxFn / PoolMaxMeanFn / column_stats;
csrc/train_paconv.hip through train_paconv.GroupFn / CenterDiffFn / SoftmaxFn / AssignFn / InterpFn): forward and
backward element-wise against the plain fp64 references of tests/embed_ops_ref.py (pinned to the oracle by test_oracle_embed_ops.py).

Gate (embed_ops_ref.gate): per tensor err = max |hip - f64| / max(1e-2, max |f64|) < max(5e-6, 3 e32) with e32 the error of the same
reference run in eager fp32 on the CPU, measured in the test.  The arg-max and the LeakyReLU kink are discontinuous, so every case asserts
on the host, before a kernel runs, that its inputs decide both by more than 32 fp32 ulps of max |u| (embed_ops_ref.undecided == 0).

Kernel -> test:
  edge_stats_kernel, edge_stats_reduce_kernel   test_bn_max_matches_fp64, test_statistics_of_a_badly_conditioned_channel, test_column_stats
  edge_fwd_kernel, edge_bwd_prep_kernel         test_bn_max_matches_fp64 (uint8 arg-max: e8_k255)
  edge_bwd_scatter_kernel                       test_bn_max_matches_fp64 (dQ; dP of the index-free cases), test_scatter_against_gather (atomics)
  edge_bwd_gather_kernel                        test_bn_max_matches_fp64 (indexed cases), test_scatter_against_gather
  pool_train_fwd_kernel, pool_train_bwd_kernel  test_pool_max_mean_matches_fp64
  softmax_fwd_kernel, softmax_bwd_kernel        test_softmax_matches_fp64
  assign_fwd_kernel, assign_bwd_kernel          test_assign_matches_fp64
  centerdiff_fwd_kernel, centerdiff_bwd_kernel  test_centerdiff_matches_fp64 (backward also under test_group_matches_fp64)
  rows_gather_bwd_kernel                        test_group_matches_fp64 (unweighted), test_interp_matches_fp64 (weighted, 3 edges per row)
  interp_fwd_kernel                             test_interp_matches_fp64
  paconv_group_kernel (paconv.hip)              test_group_matches_fp64
(three_nn_kernel is covered by the whole-path PAConv tests.)"""

import pytest
import torch
import torch.nn.functional as F

import embed_ops_ref as R
from flowcompare_amd import engine
from flowcompare_amd import train_ops as T
from flowcompare_amd import train_paconv as TP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
JUNK_SEED = 1234


def _pad(n):
    return T._round_up(n, T.ROW_PAD)


def _panel(x2d, ld, junk=0.0, rows_pad=None):
    """[rows, c] (CPU) -> device panel [rows padded to 256, ld], zero pad columns; pad rows 0 or junk * randn + junk."""
    rows, c = x2d.shape
    p = torch.zeros(rows_pad or _pad(rows), ld)
    p[:rows, :c] = x2d
    if junk:
        p[rows:] = junk * torch.randn(p.shape[0] - rows, ld, generator=torch.Generator().manual_seed(JUNK_SEED)) + junk
    return p.to(DEV)


def _dirty(*shape):
    """Leaves 7.0 in a freed block of this shape: the next torch.empty of the size gets it back, so an element a kernel skips shows."""
    t = torch.full(shape, 7.0, device=DEV)
    del t


def _zero(t):
    return t.numel() == 0 or (t == 0).all().item()


# ================================================================ BatchNorm(batch statistics) + LeakyReLU + max: train_edge.hip
def _edge_stats(pq, has_q, idx, rows, k, C, eps=R.EPS):
    """fc_train_edge_stats_f32 on a panel as BatchNormMaxFn calls it -> (mean [C], biased var [C])"""
    L = engine.lib()
    stats = torch.empty(3 * C, dtype=torch.float32, device=DEV)
    nb = L.fc_train_edge_ws_bytes(rows, C)
    ws = T._ws(nb, torch.device(DEV))
    ld = pq.shape[1]
    q_ptr = pq.data_ptr() + 4 * C if has_q else None
    L.fc_train_edge_stats_f32(engine._ptr(pq), ld, q_ptr, ld, engine._ptr(idx), rows, k, C, eps, engine._ptr(stats), engine._ptr(ws), nb, engine._stream())
    return stats[:C].clone(), stats[2 * C:].clone()


def _bn_module(c, momentum):
    bn = torch.nn.BatchNorm1d(c["C"], eps=R.EPS, momentum=momentum).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(c["gamma"])
        bn.bias.copy_(c["beta"])
        bn.running_mean.copy_(c["running_mean"])
        bn.running_var.copy_(c["running_var"])
    return bn.train()


def _run_bn_max(c, junk=0.0, momentum=0.1, steps=1):
    """One case through its autograd Function (`steps` forward passes, one backward): slope 0.2 with random indices or none ->
    train_ops.edge_bn_max; identity groups, slope 0 or a module narrower than the panel -> train_paconv.bn_act."""
    rows, k, C, ld = c["rows"], c["k"], c["C"], c["ld"]
    groups, c16 = c["variant"] == "groups", c["variant"] == "c16"
    has_q = c["Q"] is not None
    Cp = 32 if c16 else C                                               # the panel's channel count
    n_src = c["P"].shape[0]
    x = torch.zeros(n_src, ld)
    x[:, :C] = c["P"]
    if has_q:
        x[:, C:2 * C] = c["Q"]
    pq = _panel(x, ld, junk).requires_grad_(True)
    idx = None if (c["idx"] is None or groups) else c["idx"].to(DEV)
    bn = _bn_module(c, momentum)
    for _ in range(steps):
        if groups or c16 or c["slope"] != 0.2:
            out = TP.bn_act(pq, bn, rows, Cp, k=max(k, 1), slope=c["slope"])
        else:
            out = T.edge_bn_max(pq, bn, idx, rows, C, max(k, 1))
    dy = torch.zeros(rows, Cp)
    dy[:, :C] = c["dy"]
    if c16:                                                             # zero-padded channels: whatever arrives there must go nowhere
        dy[:, C:] = torch.randn(rows, Cp - C, generator=torch.Generator().manual_seed(JUNK_SEED + 1))
    out.backward(_panel(dy, Cp, junk, rows_pad=out.shape[0]))
    stat_idx = torch.arange(rows * k, dtype=torch.int32, device=DEV).view(rows, k) if groups else idx
    mean, var = _edge_stats(pq.detach(), has_q, stat_idx, rows, max(k, 1), Cp)
    r = dict(out=out.detach()[:rows, :C], dP=pq.grad[:n_src, :C], dgamma=bn.weight.grad, dbeta=bn.bias.grad, mean=mean[:C], var=var[:C],
             rmean=bn.running_mean.clone(), rvar=bn.running_var.clone())
    if has_q:
        r["dQ"] = pq.grad[:rows, C:2 * C]
    used = 2 * C if has_q else C
    pads = dict(out_rows=out.detach()[rows:], out_cols=out.detach()[:, C:], grad_rows=pq.grad[n_src:], grad_cols=pq.grad[:, used:])
    return r, pads, int(bn.num_batches_tracked)


def _bn_max_refs(c, momentum=0.1, steps=1):
    """fp64 reference and its fp32 CPU run of a case, running statistics after `steps` steps included; asserts the case is decided."""
    refs = []
    for dtype in (torch.float64, torch.float32):
        r = R.run_edge_ref(c, dtype)
        y = c["P"].to(dtype)
        if c["idx"] is not None:
            y = y[c["idx"].long()] + (c["Q"].to(dtype)[:, None] if c["Q"] is not None else 0)
        r["rmean"], r["rvar"], r["nbt"] = R.bn_running_ref(y.reshape(-1, c["C"]), c["running_mean"], c["running_var"], 0, momentum, steps)
        refs.append(r)
    m = refs[0]["margins"]
    assert R.undecided(m) == 0, "inputs leave an arg-max or a LeakyReLU branch within fp32 error: pick another seed"
    return refs


@pytest.fixture(scope="module")
def bn_refs():
    cache = {}

    def get(name):
        if name not in cache:
            c = R.make_edge_case(name)
            cache[name] = (c, *_bn_max_refs(c))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(R.EDGE_CASES))
def test_bn_max_matches_fp64(name, bn_refs):
    c, r64, r32 = bn_refs(name)
    hip, pads, nbt = _run_bn_max(c)
    R.gate(name, hip, r64, r32)
    assert nbt == r64["nbt"] == 1
    for what, t in pads.items():
        assert _zero(t), f"{name}: {what} not exactly zero"
    if c["variant"] == "orphan":                                        # no edge points at the row: an empty sum, exactly 0 on both sides
        assert _zero(r64["dP"][R.ORPHAN_ROW]) and _zero(hip["dP"][R.ORPHAN_ROW])
        assert not (c["idx"] == R.ORPHAN_ROW).any()
    if c["variant"] == "late":                                          # arg-max indices that need the uint8's top bit
        assert (r64["margins"]["jstar"] >= 128).sum() >= c["C"] // 2
    if c["variant"] == "dup":
        assert (c["idx"][:, 1] == c["idx"][:, 0]).all() and (c["idx"][::3, 3] == c["idx"][::3, 2]).all()


def test_more_than_255_neighbours_is_refused():
    c = R.make_edge_case("e8_k255")
    rows, C = c["rows"], c["C"]
    pq = _panel(torch.randn(rows, 2 * C), 2 * C)
    idx = torch.zeros(rows, 256, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="k <= 255"):
        T.edge_bn_max(pq, _bn_module(c, 0.1), idx, rows, C, 256)


@pytest.mark.parametrize("name", ["e300_dup", "e257", "e70_wide", "n300", "g64_k32_relu", "n300_c16"])
def test_bn_max_is_bit_reproducible_and_ignores_pad_rows(name):
    c = R.make_edge_case(name)
    runs = [_run_bn_max(c, junk) for junk in (0.0, 0.0, 7.0)]              # twice the same, then junk in the pad rows of input and gradient
    for r, pads, _ in runs[1:]:
        for key, t in runs[0][0].items():
            assert torch.equal(t, r[key]), f"{name}: {key} differs between runs"
        for what, t in pads.items():
            assert _zero(t), f"{name}: {what} not exactly zero"


def test_scatter_against_gather():
    """dP of one indexed case through the C ABI both ways: float atomics into a zeroed dP, and the owner-computes sum over the sorted
    edges.  They differ in summation order only: both meet the fp64 gate, and dQ is the same bits whether or not dP is asked for."""
    name = "e300"
    c = R.make_edge_case(name)
    r64, r32 = _bn_max_refs(c)
    L = engine.lib()
    rows, k, C, ld = c["rows"], c["k"], c["C"], c["ld"]
    rows_pad = _pad(rows)
    pq = _panel(torch.cat((c["P"], c["Q"]), 1), ld)
    idx = c["idx"].to(DEV)
    g32, b32 = c["gamma"].to(DEV), c["beta"].to(DEV)
    gdy = _panel(c["dy"], C)
    q_ptr = pq.data_ptr() + 4 * C
    s = engine._stream()
    stats = torch.empty(3 * C, dtype=torch.float32, device=DEV)
    out = torch.zeros(rows_pad, C, device=DEV)
    arg = torch.empty(rows, C, dtype=torch.uint8, device=DEV)
    nb = L.fc_train_edge_ws_bytes(rows, C)
    ws = T._ws(nb, torch.device(DEV))
    common = (engine._ptr(pq), ld, q_ptr, ld, engine._ptr(idx), rows, k, C, engine._ptr(stats))
    L.fc_train_edge_stats_f32(*common[:8], R.EPS, engine._ptr(stats), engine._ptr(ws), nb, s)
    L.fc_train_edge_fwd_f32(*common, engine._ptr(g32), engine._ptr(b32), 0.2, engine._ptr(out), C, engine._ptr(arg), s)
    t1, t2 = torch.empty(rows_pad, C, device=DEV), torch.empty(rows_pad, C, device=DEV)
    L.fc_train_edge_bwd_prep_f32(*common, engine._ptr(g32), engine._ptr(b32), 0.2, engine._ptr(arg), engine._ptr(gdy), C,
                                 engine._ptr(t1), engine._ptr(t2), C, rows_pad, s)
    dbeta, dgamma = T._colsum(t1, C, rows), T._colsum(t2, C, rows)
    tail = (engine._ptr(g32), engine._ptr(arg), engine._ptr(t1), C, engine._ptr(dbeta), engine._ptr(dgamma))
    d_sc, d_ga = torch.zeros(rows_pad, ld, device=DEV), torch.zeros(rows_pad, ld, device=DEV)
    L.fc_train_edge_bwd_scatter_f32(*common, *tail, engine._ptr(d_sc), ld, d_sc.data_ptr() + 4 * C, ld, s)
    L.fc_train_edge_bwd_scatter_f32(*common, *tail, None, ld, d_ga.data_ptr() + 4 * C, ld, s)
    order, offsets = T._sorted_edges(idx, rows)
    L.fc_train_edge_bwd_gather_f32(*common, *tail, engine._ptr(order), engine._ptr(offsets), engine._ptr(d_ga), ld, s)
    for tag, d in (("scatter (atomics)", d_sc), ("gather (sorted)", d_ga)):
        R.gate(f"{name} {tag}", dict(out=out[:rows], dP=d[:rows, :C], dQ=d[:rows, C:2 * C], dgamma=dgamma, dbeta=dbeta), r64, r32)
    assert torch.equal(d_sc[:, C:2 * C], d_ga[:, C:2 * C])
    assert _zero(d_sc[rows:]) and _zero(d_ga[rows:]) and _zero(d_sc[:, 2 * C:]) and _zero(d_ga[:, 2 * C:])


def _stats_yardstick(y2d):
    """mean and biased variance: fp64, and CPU fp32 F.batch_norm (momentum 1: its running statistics are the batch's, variance unbiased)"""
    n, C = y2d.shape
    y64 = y2d.double()
    r64 = dict(mean=y64.mean(0), var=y64.var(0, unbiased=False))
    rm, rv = torch.zeros(C), torch.ones(C)
    F.batch_norm(y2d.float(), rm, rv, training=True, momentum=1.0, eps=R.EPS)
    return r64, dict(mean=rm, var=rv * ((n - 1) / n))


def test_statistics_of_a_badly_conditioned_channel():
    """One channel of P shifted by +1000 at unit spread: sum of squares 1e6 times the variance.  fp64 accumulators keep mean and variance."""
    c = R.make_edge_case("e300")
    rows, k, C, ld = c["rows"], c["k"], c["C"], c["ld"]
    P = c["P"].clone()
    P[:, 3] += 1000.0
    pq = _panel(torch.cat((P, c["Q"]), 1), ld, junk=7.0)
    mean, var = _edge_stats(pq, True, c["idx"].to(DEV), rows, k, C)
    y = (P[c["idx"].long()] + c["Q"][:, None]).reshape(-1, C)             # the fp32 sums the kernel reads, exactly
    r64, r32 = _stats_yardstick(y)
    R.gate("shifted channel, indexed", dict(mean=mean, var=var), r64, r32)
    err3 = abs(var[3].item() - r64["var"][3].item()) / r64["var"][3].item()
    print(f"shifted channel alone: var {var[3].item():.6f} vs {r64['var'][3].item():.6f} (rel {err3:.1e})")
    assert err3 < 5e-6                                                   # the channel itself, not only the tensor's maximum


@pytest.mark.parametrize("rows,width,ld", [(1000, 96, 128), (70, 35, 64)])
def test_column_stats(rows, width, ld):
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, width, generator=g) * (0.5 + torch.rand(width, generator=g)) + torch.randn(width, generator=g)
    x[:, 1] += 1000.0
    mean, var = T.column_stats(_panel(x, ld, junk=7.0), width, rows)
    r64, r32 = _stats_yardstick(x)
    R.gate(f"column_stats rows {rows} width {width}", dict(mean=mean, var=var), r64, r32)


@pytest.mark.parametrize("momentum", [0.1, 0.3, None])
@pytest.mark.parametrize("name", ["e70_wide", "n300_c16", "g64_k32_relu"])
def test_running_statistics_follow_torch_over_two_steps(name, momentum):
    """running_mean, running_var (unbiased, n = rows k) and num_batches_tracked after two train-mode steps, for a fixed momentum and for
    momentum=None (torch: cumulative average, factor 1 / num_batches_tracked after the increment).  n300_c16: a 16-channel module in a
    32-wide panel, whose buffers take the first 16 channels' statistics."""
    c = R.make_edge_case(name)
    r64, r32 = _bn_max_refs(c, momentum, steps=2)
    hip, _, nbt = _run_bn_max(c, momentum=momentum, steps=2)
    assert hip["rmean"].shape == hip["rvar"].shape == (c["C"],)
    R.gate(f"{name} momentum {momentum}", dict(rmean=hip["rmean"], rvar=hip["rvar"]), r64, r32)
    assert nbt == r64["nbt"] == 2


# ================================================================ global pooling
def _run_pool(name):
    B, M, width, ld, _ = R.POOL_CASES[name]
    t, dy, _ = R.make_pool_case(name)
    tp = _panel(t.reshape(B * M, width), ld, junk=7.0).requires_grad_(True)
    out = T.pool_max_mean(tp, B, M, width)
    out.backward(dy.to(DEV))
    return dict(out=out.detach(), dt=tp.grad[:B * M, :width]), tp.grad


@pytest.mark.parametrize("name", list(R.POOL_CASES))
def test_pool_max_mean_matches_fp64(name):
    B, M, width, ld, _ = R.POOL_CASES[name]
    t, dy, _ = R.make_pool_case(name)
    assert R.undecided(R.pool_margins(t.double())) == 0
    refs = []
    for dtype in (torch.float64, torch.float32):
        x = t.detach().to(dtype).clone().requires_grad_(True)
        o = R.pool_max_mean_ref(x)
        o.backward(dy.to(dtype))
        refs.append(dict(out=o.detach(), dt=x.grad.reshape(B * M, width)))
    hip, grad = _run_pool(name)
    R.gate(name, hip, *refs)
    assert _zero(grad[B * M:]) and _zero(grad[:, width:])
    again, _ = _run_pool(name)
    assert all(torch.equal(hip[k], again[k]) for k in hip)
    if name.endswith("_tie"):                                           # rows 31 and 150 of scene 1 are equal and maximal: the lower index takes the gradient
        want = dy[1, :width] + dy[1, width:] / M
        assert torch.allclose(hip["dt"][M + 31].cpu(), want, rtol=1e-6, atol=0)
        assert torch.equal(hip["dt"][M + 150].cpu(), (dy[1, width:] / M))


# ================================================================ PAConv operators: train_paconv.hip
def _both(fn, inputs, dy):
    """fn on float inputs (a dict; integer tensors pass through) in fp64 and in fp32 on the CPU -> two dicts: out and d<name> per input."""
    refs = []
    for dtype in (torch.float64, torch.float32):
        x = {k: v.detach().to(dtype).clone().requires_grad_(True) if v.is_floating_point() else v for k, v in inputs.items()}
        out = fn(**x)
        out.backward(dy.to(dtype))
        r = {"out": out.detach()}
        r.update({"d" + k: v.grad for k, v in x.items() if v.is_floating_point()})
        refs.append(r)
    return refs


@pytest.mark.parametrize("rows,width,ld,scale", [(300, 8, 32, 1.0), (1000, 8, 32, 1.0), (300, 32, 32, 1.0), (300, 8, 32, 80.0)])
def test_softmax_matches_fp64(rows, width, ld, scale):
    g = torch.Generator().manual_seed(rows + width)
    x = torch.randn(rows, width, generator=g) if scale == 1.0 else (torch.rand(rows, width, generator=g) * 2 - 1) * scale
    dy = torch.randn(rows, width, generator=g)
    r64, r32 = _both(R.softmax_ref, dict(x=x), dy)
    xp = _panel(x, ld, junk=7.0).requires_grad_(True)
    _dirty(*xp.shape)
    y = TP.SoftmaxFn.apply(xp, width, rows)
    _dirty(*xp.shape)
    y.backward(_panel(dy, ld, junk=7.0))
    R.gate(f"softmax rows {rows} width {width} scale {scale}", dict(out=y.detach()[:rows, :width], dx=xp.grad[:rows, :width]), r64, r32)
    for t in (y.detach(), xp.grad):
        assert _zero(t[rows:]) and _zero(t[:, width:])


def _run_assign(G, S, dy, rows, m, Cout):
    Gp, Sp = _panel(G, m * Cout, junk=7.0).requires_grad_(True), _panel(S, 32, junk=7.0).requires_grad_(True)
    _dirty(Gp.shape[0], TP._r32(Cout))
    out = TP.AssignFn.apply(Gp, Sp, m, Cout, rows)
    _dirty(*Gp.shape)
    _dirty(*Sp.shape)
    out.backward(_panel(dy, TP._r32(Cout), junk=7.0))
    return out.detach(), Gp.grad, Sp.grad


@pytest.mark.parametrize("rows,m,Cout", [(300, 8, 32), (515, 8, 96), (70, 8, 64)])
def test_assign_matches_fp64(rows, m, Cout):
    g = torch.Generator().manual_seed(rows)
    G = torch.randn(rows, m * Cout, generator=g)
    S = torch.softmax(torch.randn(rows, m, generator=g), -1)
    dy = torch.randn(rows, Cout, generator=g)
    r64, r32 = _both(R.assign_ref, dict(S=S, G=G), dy)
    out, dG, dS = _run_assign(G, S, dy, rows, m, Cout)
    R.gate(f"assign rows {rows} m {m} Cout {Cout}", dict(out=out[:rows, :Cout], dG=dG[:rows], dS=dS[:rows, :m]), r64, r32)
    assert _zero(out[rows:]) and _zero(out[:, Cout:]) and _zero(dG[rows:]) and _zero(dS[rows:]) and _zero(dS[:, m:])
    again = _run_assign(G, S, dy, rows, m, Cout)
    assert all(torch.equal(a, b) for a, b in zip((out, dG, dS), again))


@pytest.mark.parametrize("groups,K,C,ld", [(9, 32, 64, 64), (70, 4, 35, 96), (5, 32, 3, 32)])
def test_centerdiff_matches_fp64(groups, K, C, ld):
    g = torch.Generator().manual_seed(groups)
    rows = groups * K
    x = torch.randn(rows, C, generator=g)
    dy = torch.randn(rows, 2 * C, generator=g)
    r64, r32 = _both(lambda x: R.centerdiff_ref(x, K), dict(x=x), dy)
    wide = torch.randn(rows, ld, generator=g)                            # a panel wider than C: its other columns are someone else's data
    wide[:, :C] = x
    xp = _panel(wide, ld, junk=7.0).requires_grad_(True)
    E = TP.CenterDiffFn.apply(xp, C, K, groups)
    assert E.shape == (_pad(rows), TP._r32(2 * C))
    _dirty(*xp.shape)
    E.backward(_panel(dy, E.shape[1], junk=7.0))
    R.gate(f"centerdiff groups {groups} K {K} C {C}", dict(out=E.detach()[:rows, :2 * C], dx=xp.grad[:rows, :C]), r64, r32)
    assert _zero(E.detach()[rows:]) and _zero(E.detach()[:, 2 * C:]) and _zero(xp.grad[rows:]) and _zero(xp.grad[:, C:])


def _run_group(feat, xyz4, qxyz4, dE, B, n, m, K, C):
    fp = _panel(feat, 32, junk=7.0).requires_grad_(True)
    xd, qd = xyz4.to(DEV), qxyz4.to(DEV)
    nidx = torch.empty(B * m, K, dtype=torch.int32, device=DEV)
    engine.lib().fc_op_paconv_knn_f32(engine._ptr(xd), engine._ptr(qd), engine._ptr(nidx), B, n, m, K, engine._stream())
    E, gdiff = TP.GroupFn.apply(fp, xd, qd, nidx, C, B, n, m)
    E.backward(_panel(dE, E.shape[1], junk=7.0))
    return E.detach(), gdiff, fp.grad, nidx.cpu()


@pytest.mark.parametrize("B,n,m,K,C", [(2, 64, 16, 32, 6), (1, 20, 5, 32, 3)])
def test_group_matches_fp64(B, n, m, K, C):
    g = torch.Generator().manual_seed(n)
    xyz = torch.randn(B, n, 3, generator=g)
    if n > K:
        xyz[:, -16:] += 10.0                                             # a far cluster: in no query's neighbourhood, so no edge points at it
    xyz4 = torch.zeros(B * n, 4)
    xyz4[:, :3] = xyz.reshape(B * n, 3)
    qxyz4 = xyz4.view(B, n, 4)[:, :m].reshape(B * m, 4).contiguous()     # the queries are the first m points of each scene
    feat = torch.randn(B * n, C, generator=g)
    edges, w = B * m * K, 2 * (C + 3)
    dE = torch.randn(edges, w, generator=g)
    E, gdiff, dfeat, nidx = _run_group(feat, xyz4, qxyz4, dE, B, n, m, K, C)
    assert nidx.min() >= 0 and nidx.max() < n
    if n < K:
        assert (nidx[:, n:] == 0).all()                                  # fewer points than neighbours: the tail repeats index 0
    r64, r32 = [], []
    for dtype, dst in ((torch.float64, r64), (torch.float32, r32)):
        f = feat.detach().to(dtype).clone().requires_grad_(True)
        Er, gr = R.group_ref(f, xyz4[:, :3].to(dtype), qxyz4[:, :3].to(dtype), nidx, B, n, m)
        Er.backward(dE.to(dtype))
        dst.append(dict(E=Er.detach(), gdiff=gr, dfeat=f.grad))
    r64, r32 = r64[0], r32[0]
    R.gate(f"group B {B} n {n} m {m} K {K} C {C}", dict(E=E[:edges, :w], gdiff=gdiff[:edges, :3], dfeat=dfeat[:B * n, :C]), r64, r32)
    assert _zero(E[edges:]) and _zero(E[:, w:]) and _zero(gdiff[edges:]) and _zero(gdiff[:, 3:])
    assert _zero(dfeat[B * n:]) and _zero(dfeat[:, C:])
    used = torch.bincount((nidx.long() + (torch.arange(B * m) // m * n)[:, None]).reshape(-1), minlength=B * n)
    if n > K:
        assert (used == 0).any() and _zero(dfeat[:B * n][used == 0])     # empty edge lists
    assert used.max() > 8                                                # ... and long ones
    again = _run_group(feat, xyz4, qxyz4, dE, B, n, m, K, C)
    assert all(torch.equal(a, b) for a, b in zip((E, gdiff, dfeat, nidx), again))


def _run_interp(Fk, idx, w, dy, rows, C, ld):
    fp = _panel(Fk, ld, junk=7.0).requires_grad_(True)
    _dirty(_pad(rows), TP._r32(C))
    out = TP.InterpFn.apply(fp, idx.to(DEV), w.to(DEV), C, rows)
    _dirty(*fp.shape)
    out.backward(_panel(dy, TP._r32(C), junk=7.0))
    return out.detach(), fp.grad


@pytest.mark.parametrize("rows,n_known,C,ld", [(300, 75, 64, 64), (20, 2, 35, 96)])
def test_interp_matches_fp64(rows, n_known, C, ld):
    g = torch.Generator().manual_seed(rows)
    Fk = torch.randn(n_known, C, generator=g)
    idx = torch.randint(0, n_known, (rows, 3), generator=g, dtype=torch.int32)
    idx[5] = idx[5, 0]                                                   # all three neighbours coincide
    lonely = 7 if n_known > 7 else None
    if lonely is not None:
        idx[idx == lonely] = lonely + 1                                  # a known row no edge points at
    w = torch.rand(rows, 3, generator=g) + 0.05
    w = w / w.sum(-1, keepdim=True)
    dy = torch.randn(rows, C, generator=g)
    r64, r32 = _both(lambda Fk, w: R.interp_ref(Fk, idx, w), dict(Fk=Fk, w=w), dy)
    out, dF = _run_interp(Fk, idx, w, dy, rows, C, ld)
    R.gate(f"interp rows {rows} known {n_known} C {C}", dict(out=out[:rows, :C], dFk=dF[:n_known, :C]), r64, r32)
    assert _zero(out[rows:]) and _zero(out[:, C:]) and _zero(dF[n_known:]) and _zero(dF[:, C:])
    if lonely is not None:
        assert _zero(dF[lonely]) and _zero(r64["dFk"][lonely])
    again = _run_interp(Fk, idx, w, dy, rows, C, ld)
    assert torch.equal(out, again[0]) and torch.equal(dF, again[1])
