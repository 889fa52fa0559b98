"""Plain differentiable torch references of the embedder training operators (csrc/train_edge.hip, csrc/train_paconv.hip), the inputs of
the operator tests and the gate they share.  Everything works on dense [rows, C] tensors and explicit index tensors in whatever dtype it
is given: fp64 is the reference, the same function in fp32 on the CPU is the yardstick (tests/test_gpu_train_embed_ops.py).  Written from
the formulae in the kernel headers; tests/test_oracle_embed_ops.py pins every function to oracle/ on the CPU."""
import torch
import torch.nn.functional as F

EPS = 1e-5


# ---------------------------------------------------------------- references
def edge_bn_max_ref(P, Q, idx, gamma, beta, slope, eps=EPS):
    """y_ij = P[idx_ij] + Q[i] (y = P[:, None] without idx; Q may be None) -> BatchNorm with the biased statistics over every (i, j)
    -> LeakyReLU(slope) -> max over j.  Returns (out [rows, C], mean [C], biased var [C], margins) -- see `edge_margins`."""
    if idx is None:
        y = P[:, None]
    else:
        y = P[idx.long()]
        if Q is not None:
            y = y + Q[:, None]
    mean, var = y.mean((0, 1)), y.var((0, 1), unbiased=False)
    u = (y - mean) * torch.rsqrt(var + eps) * gamma + beta
    z = F.leaky_relu(u, slope)
    out = z.max(dim=1)[0]
    return out, mean, var, edge_margins(u.detach(), z.detach(), idx, slope)


def edge_margins(u, z, idx, slope):
    """What decides an fp32 kernel's discontinuous choices on u, z [rows, k, C] (fp64):
         tau    32 * 2^-24 * max |u|: the size of an fp32 kernel's error on u, with margin
         gap    per (i, c): best z minus the best z among the edges whose SOURCE ROW differs from the arg-max's (two edges of one source
                carry the same y, and either choice gives the same gradients); +inf where no such edge exists.  With slope == 0 only
                where the best z is positive (below, every edge has derivative 0 and the choice is immaterial)
         ustar  per (i, c): max_j u, the pre-activation at the arg-max (LeakyReLU is monotone): its sign picks the derivative 1 or slope
         jstar  per (i, c): the first j that attains the maximum (what a strict `>` scan keeps)"""
    rows, k, C = u.shape
    tau = 32 * 2.0 ** -24 * u.abs().max().item()
    zb, jb = z.max(dim=1)
    src = (idx.long() if idx is not None else torch.arange(rows)[:, None])[:, :, None].expand(rows, k, C)
    src_best = torch.gather(src, 1, jb[:, None, :])
    other = torch.where(src != src_best, z, torch.full_like(z, float("-inf")))
    gap = zb - other.max(dim=1)[0]
    if slope == 0:
        gap = torch.where(zb > 0, gap, torch.full_like(gap, float("inf")))
    jstar = torch.where(z == zb[:, None], torch.arange(k)[None, :, None], k).min(dim=1)[0]
    return dict(tau=tau, gap=gap, ustar=u.max(dim=1)[0], jstar=jstar)


def undecided(margins):
    """Number of (i, c) entries whose arg-max or LeakyReLU branch an fp32 error of tau could flip (must be 0: nothing is left out)."""
    return int((margins["gap"] < margins["tau"]).sum() + (margins["ustar"].abs() < margins["tau"]).sum())


def bn_running_ref(y2d, running_mean, running_var, num_batches_tracked, momentum, steps=1, eps=EPS):
    """`steps` train-mode steps of torch.nn.BatchNorm1d on y2d [n, C] in y2d's dtype -> (running_mean, running_var, num_batches_tracked)."""
    bn = torch.nn.BatchNorm1d(y2d.shape[1], eps=eps, momentum=momentum).to(y2d.dtype)
    with torch.no_grad():
        bn.running_mean.copy_(running_mean)
        bn.running_var.copy_(running_var)
        bn.num_batches_tracked.fill_(int(num_batches_tracked))
        bn.train()
        for _ in range(steps):
            bn(y2d)
    return bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)


def pool_max_mean_ref(t):
    """t [B, M, width] -> [B, 2 width] = [max over M | mean over M] (torch.max: the gradient goes to the FIRST maximal row)."""
    return torch.cat((t.max(dim=1)[0], t.mean(dim=1)), -1)


def pool_margins(t):
    """tau and, per (b, c), the gap between the maximum and the largest DIFFERENT value (exactly equal rows are one decision under the
    first-index rule both sides state)."""
    tau = 32 * 2.0 ** -24 * t.abs().max().item()
    mx = t.max(dim=1, keepdim=True)[0]
    other = torch.where(t != mx, t, torch.full_like(t, float("-inf")))
    return dict(tau=tau, gap=(mx - other.max(dim=1, keepdim=True)[0])[:, 0], ustar=torch.full_like(mx[:, 0], float("inf")))


def softmax_ref(x):
    return torch.softmax(x, dim=-1)


def assign_ref(S, G):
    """out[e, o] = sum_m S[e, m] G[e, m Cout + o]"""
    e, m = S.shape
    return torch.einsum("em,emo->eo", S, G.reshape(e, m, -1))


def centerdiff_ref(x, K):
    """x [groups K, C] -> [x_e - x_centre | x_e], centre = row 0 of each group of K consecutive rows."""
    xg = x.reshape(-1, K, x.shape[1])
    return torch.cat((xg - xg[:, :1], xg), -1).reshape(-1, 2 * x.shape[1])


def group_ref(feat, xyz, qxyz, nidx, B, n, m):
    """feat [B n, C], xyz [B n, 3], qxyz [B m, 3], nidx [B m, K] indices inside the scene ->
    E [B m K, 2 (C + 3)] = [x_e - x_0 | x_e] with x_e = [xyz[idx_e] - qxyz | feat[idx_e]], gdiff [B m K, 3] = xyz[idx_e] - xyz[idx_0]."""
    K = nidx.shape[1]
    src = nidx.long() + (torch.arange(B * m) // m * n)[:, None]
    xe = torch.cat((xyz[src] - qxyz[:, None], feat[src]), -1)
    E = torch.cat((xe - xe[:, :1], xe), -1).reshape(B * m * K, -1)
    gdiff = (xyz[src] - xyz[src[:, :1]]).reshape(B * m * K, 3)
    return E, gdiff


def interp_ref(Fk, idx, w):
    """(w0 f0 + w1 f1) + w2 f2 with f_r = Fk[idx[:, r]]"""
    i = idx.long()
    return (w[:, 0:1] * Fk[i[:, 0]] + w[:, 1:2] * Fk[i[:, 1]]) + w[:, 2:3] * Fk[i[:, 2]]


# ---------------------------------------------------------------- the gate
def rel(a, b, floor=1e-2):
    """max |a - b| relative to max |b|, floored (tests/test_gpu_train.py _rel)."""
    return (a.detach().double().cpu() - b.detach()).abs().max().item() / max(floor, b.detach().abs().max().item())


def gate(tag, hip, f64, f32):
    """Every tensor of `hip` within max(5e-6, 3 x the error of the same reference run in eager fp32 on the CPU) of fp64.
    5e-6: the project's gate for fp32 row kernels; 3: its margin over eager fp32 for a different summation order."""
    bad, cells = [], []
    for name in hip:
        err, e32 = rel(hip[name], f64[name]), rel(f32[name], f64[name])
        cells.append(f"{name} {err:.1e}/{e32:.1e}")
        if not err < max(5e-6, 3 * e32):
            bad.append((name, err, e32))
    print(f"{tag}: err/e32  " + "  ".join(cells))
    assert not bad, f"{tag}: {bad}"


# ---------------------------------------------------------------- inputs of the BatchNorm + max tests
# name -> rows, k, C, panel width, slope, variant, seed.  k == 0: no index (y = P, one value per row).  Variants: "dup" idx[:, 1] = idx[:, 0]
# and every third row a second duplicate; "orphan" one row index removed from idx; "groups" identity indices over groups of k consecutive
# rows and no Q (train_paconv.bn_act); "late" row i meets source i only from neighbour 200 on, so where that source wins the arg-max
# needs all 8 bits; "c16" a 16-channel BatchNorm in a 32-wide panel.  Seeds: the first of 0, 1, 2, ... at which
# `undecided` is 0 (test_oracle_embed_ops.py checks every one of them on the CPU).
EDGE_CASES = {
    "e300": dict(rows=300, k=20, C=64, ld=128, slope=0.2, variant=None, seed=0),
    "e257": dict(rows=257, k=20, C=128, ld=256, slope=0.2, variant=None, seed=6),
    "e70_wide": dict(rows=70, k=5, C=32, ld=96, slope=0.2, variant=None, seed=0),
    "e1000": dict(rows=1000, k=7, C=96, ld=192, slope=0.2, variant=None, seed=95),
    "e300_dup": dict(rows=300, k=20, C=64, ld=128, slope=0.2, variant="dup", seed=0),
    "e300_orphan": dict(rows=300, k=20, C=64, ld=128, slope=0.2, variant="orphan", seed=0),
    "e8_k255": dict(rows=8, k=255, C=32, ld=64, slope=0.2, variant="late", seed=0),
    "n300": dict(rows=300, k=0, C=96, ld=96, slope=0.2, variant=None, seed=0),
    "n1000_relu": dict(rows=1000, k=0, C=32, ld=32, slope=0.0, variant=None, seed=0),
    "g64_k32_relu": dict(rows=64, k=32, C=64, ld=64, slope=0.0, variant="groups", seed=0),
    "n300_c16": dict(rows=300, k=0, C=16, ld=32, slope=0.0, variant="c16", seed=0),
}
ORPHAN_ROW = 17
LATE_FROM = 200


def make_edge_case(name, seed=None):
    """fp32 inputs of one case: P (and Q, idx), gamma in [0.5, 1.5] with every 5th channel negated, beta ~ 0.3 N(0, 1), the upstream
    gradient dy and the BatchNorm module's running statistics before the step."""
    c = dict(EDGE_CASES[name])
    g = torch.Generator().manual_seed(c["seed"] if seed is None else seed)
    rows, k, C = c["rows"], c["k"], c["C"]
    groups = c["variant"] == "groups"
    n_src = rows * k if groups else rows
    c["P"] = torch.randn(n_src, C, generator=g)
    c["Q"] = torch.randn(rows, C, generator=g) if (k and not groups) else None
    c["idx"] = None
    if groups:
        c["idx"] = torch.arange(rows * k, dtype=torch.int32).view(rows, k)
    elif k:
        idx = torch.randint(0, rows, (rows, k), generator=g, dtype=torch.int32)
        if c["variant"] == "dup":
            idx[:, 1] = idx[:, 0]
            idx[::3, 3] = idx[::3, 2]
        if c["variant"] == "late":
            early = torch.randint(0, rows - 1, (rows, LATE_FROM), generator=g, dtype=torch.int32)
            idx[:, :LATE_FROM] = early + (early >= torch.arange(rows, dtype=torch.int32)[:, None]).int()
        if c["variant"] == "orphan":
            idx[idx == ORPHAN_ROW] = ORPHAN_ROW + 1
        c["idx"] = idx
    gamma = 0.5 + torch.rand(C, generator=g)
    gamma[::5] *= -1
    c["gamma"], c["beta"] = gamma, 0.3 * torch.randn(C, generator=g)
    c["dy"] = torch.randn(rows, C, generator=g)
    c["running_mean"], c["running_var"] = 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    return c


def run_edge_ref(c, dtype):
    """The reference with autograd on a case in `dtype`: dict of out, dP, dQ, dgamma, dbeta, mean, var (+ margins under "margins")."""
    cast = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_(True)
    P, Q, gamma, beta = cast(c["P"]), cast(c["Q"]), cast(c["gamma"]), cast(c["beta"])
    out, mean, var, margins = edge_bn_max_ref(P, Q, c["idx"], gamma, beta, c["slope"])
    out.backward(c["dy"].to(dtype))
    r = dict(out=out.detach(), dP=P.grad, dgamma=gamma.grad, dbeta=beta.grad, mean=mean.detach(), var=var.detach(), margins=margins)
    if Q is not None:
        r["dQ"] = Q.grad
    return r


# ---------------------------------------------------------------- inputs of the pooling tests: (B, M, width, panel width, seed)
POOL_CASES = {"p2x200": (2, 200, 96, 128, 0), "p3x5": (3, 5, 32, 64, 0), "p1x1": (1, 1, 64, 96, 0), "p2x200_tie": (2, 200, 96, 128, 0)}


def make_pool_case(name, seed=None):
    B, M, width, ld, s = POOL_CASES[name]
    g = torch.Generator().manual_seed(s if seed is None else seed)
    t = torch.randn(B, M, width, generator=g)
    if name.endswith("_tie"):
        t[1, 150] = t[1, 31] = t[1].max(dim=0)[0] + 0.5            # two equal rows that hold the maximum of every channel of scene 1
    return t, torch.randn(B, 2 * width, generator=g), ld
