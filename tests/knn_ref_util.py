"""Reference side of the DGCNN k-NN tests on ties, duplicates and degenerate clouds (tests/test_gpu_knn_degenerate.py; checked on the host by
tests/test_knn_ref_host.py).

Both kernels of csrc/knn.hip rank candidate j of query i by pd = 2 xi.xj - |xj|^2 - |xi|^2, largest first, and state one tie rule: among equal
values the candidate of LOWEST index wins.  stable_topk applies that rule to the fp64 ranking.  exact_clouds() are clouds of small integers:
every product and every partial sum of either kernel is then an integer below 2^24, i.e. exact in fp32 in whatever order it is formed, the
fp32 ranking equals the fp64 one bit for bit, and the kernels' sets must EQUAL stable_topk's -- no tolerance, ties included."""
import functools

import torch

K_MAX = 64


def ranking(f):
    """pd[b, i, j] = 2 xi.xj - |xj|^2 - |xi|^2 in fp64 for f [B, M, C]."""
    fd = f.double()
    sq = (fd ** 2).sum(-1)
    return 2 * (fd @ fd.transpose(1, 2)) - sq[:, None, :] - sq[:, :, None]


def stable_topk(f, k):
    """The k largest of ranking(f) per query, the lowest index first among equal values -> int64 [B, M, k], every set sorted by index."""
    order = torch.sort(ranking(f), dim=-1, descending=True, stable=True).indices       # stable: equal values keep their index order
    return order[..., :k].sort(-1).values


def brute_topk(f, k):
    """stable_topk as a plain Python loop over exact integers / floats (the check of the check; small clouds only)."""
    B, M, _ = f.shape
    out = torch.empty(B, M, k, dtype=torch.int64)
    rows = f.double().tolist()
    for b in range(B):
        sq = [sum(v * v for v in r) for r in rows[b]]
        for i in range(M):
            pd = [2 * sum(p * q for p, q in zip(rows[b][i], rows[b][j])) - sq[j] - sq[i] for j in range(M)]
            taken = []
            for _ in range(k):                                     # k passes: the largest value not taken yet, the first index that has it
                best = None
                for j in range(M):
                    if j not in taken and (best is None or pd[j] > pd[best]):
                        best = j
                taken.append(best)
            out[b, i] = torch.tensor(sorted(taken))
    return out


def _ints(seed, M, C, lo, hi):
    return torch.randint(lo, hi + 1, (M, C), generator=torch.Generator().manual_seed(seed)).float()


def _lattice():
    ax = torch.arange(-3, 5).float()                                # 8 x 8 x 8, the origin is a point
    return torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(512, 3)


def _scene0():
    intfeat64 = _ints(101, 300, 64, -2, 2)
    zero_cluster = intfeat64.clone()
    zero_cluster[100:170] = 0.0                                     # 70 >= K_MAX coincident points at the origin of feature space
    base = _ints(103, 80, 16, -2, 2)
    assert torch.unique(base, dim=0).shape[0] == 80
    return {
        "lattice3": _lattice(),
        "lattice6": torch.cat((_lattice(), _ints(100, 512, 3, 0, 3)), -1),
        "intfeat64": intfeat64,
        "intfeat100": _ints(102, 129, 100, -2, 2),                  # (128 channels with zero padding on the matrix-core kernel)
        "copies": base.repeat(4, 1),                                # row i and rows i + 80, i + 160, i + 240 are one point
        "zero_cluster": zero_cluster,
        "all_equal": torch.tensor([1.0, -2.0, 3.0, 0.0, 2.0, -1.0]).repeat(128, 1),
        "all_zero": torch.zeros(128, 6),
        "m_eq_k_40": _ints(104, 40, 6, -3, 3),
        "m_eq_k_64": _ints(105, 64, 64, -2, 2),
        # voxel-like coordinates and quantised colours at a size whose last workgroup, 64-candidate block and
        # 32-candidate tile are all partial (2085 = 16 * 128 + 37), every query with dozens of exact ties
        "tail2085": _ints(106, 2085, 6, -3, 4),
    }


@functools.lru_cache(maxsize=None)
def exact_clouds():
    """name -> float32 [2, M, C]; scene 1 is scene 0 with its rows reversed, so that ties meet the candidate stream in both orders."""
    out = {}
    for name, s0 in _scene0().items():
        f = torch.stack((s0, s0.flip(0)))
        assert torch.equal(f, f.round()), name
        # every value either kernel forms is a sum of products of entries bounded by 4 max |x|^2 (|pd| <= |xi|^2 + 2 |xi.xj| + |xj|^2)
        assert 4 * float((f.double() ** 2).sum(-1).max()) < 2 ** 24, name
        out[name] = f
    return out


def ks_of(name):
    """The neighbour counts of the exact-set tests: 40 and 8 everywhere, 64 where the cloud has 128 points, M itself on the M == k clouds."""
    M = exact_clouds()[name].shape[1]
    ks = {40, 8}
    if M >= 128:
        ks.add(64)
    if name.startswith("m_eq_k"):
        ks.add(M)
    return sorted(ks)


EXACT_CASES = [(name, k) for name in _scene0() for k in ks_of(name)]


@functools.lru_cache(maxsize=None)
def _exact_top(name, doubled_channel):
    f = exact_clouds()[name]
    if doubled_channel is not None:
        f = f.clone()
        f[..., doubled_channel] *= 2
    return torch.sort(ranking(f), dim=-1, descending=True, stable=True).indices[..., :K_MAX].contiguous()


def exact_sets(name, k, doubled_channel=None):
    """stable_topk of an exact cloud (one sort per cloud, shared by the tests); doubled_channel: of the same cloud with that channel doubled --
    a nearby feature space with other ties, still all integers."""
    return _exact_top(name, doubled_channel)[..., :k].sort(-1).values


def check_sets(idx, f, k, tol):
    """What can be asked of a k-NN result where rounding decides near-ties: idx [B, M, k] holds indices inside the scene, k distinct ones
    per query, and every returned candidate ranks (in fp64) no lower than the true k-th best minus tol.  Returns the worst shortfall."""
    B, M, _ = f.shape
    idx = idx.long()
    assert idx.shape == (B, M, k)
    assert int(idx.min()) >= 0 and int(idx.max()) < M, "index outside the scene"
    srt = idx.sort(-1).values
    assert bool((srt[..., 1:] != srt[..., :-1]).all()), "a set repeats an index"
    if tol is None:
        return None
    pd = ranking(f)
    kth = pd.sort(-1, descending=True).values[..., k - 1]
    short = float((kth[..., None] - torch.gather(pd, 2, idx)).max())
    assert short <= tol, f"a returned neighbour ranks {short:.3e} below the true k-th best (tolerance {tol:.3e})"
    return short


def fp32_dot_tol(f):
    """2 (C + 2) 2^-24 max(|xi|^2 + |xj|^2): the worst-case error of an fp32 ranking value (a C-term dot product and two norms, each term
    rounded once, then two subtractions), twice -- the k-th best and the returned candidate can both be off."""
    C = f.shape[-1]
    return 2 * (C + 2) * 2.0 ** -24 * 2 * float((f.double() ** 2).sum(-1).max())


# ------------------------------------------------------------------------------------------------ the embedder on degenerate clouds
def synth_cloud(M, seed):
    """One scene [1, M, 6] as tests/fullsize_util.synth_pairs draws it: xyz uniform, centred, scaled into the unit sphere; rgb ~ U[0, 1)."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(1, M, 3, generator=g) * 2 - 1
    xyz = xyz - xyz.mean(1, keepdim=True)
    xyz = xyz / xyz.norm(dim=-1).amax(1)[:, None, None]
    return torch.cat((xyz, torch.rand(1, M, 3, generator=g)), -1)


def clustered_cloud(M, seed, k=40, spread=0.01):
    """A random cloud [1, M, 6] WITHOUT ties at the k-th neighbour: M // k clusters of exactly k points (uniform within +-spread of a
    synth_cloud centre) and one of the M % k points left over, shuffled over the stream.  The k nearest of a cluster member are its
    cluster, and the (k + 1)-th is a whole inter-cluster distance further -- asserted here, in fp64, to be at least 1000 x the worst-case
    fp32 error of a ranking value, where in a uniform cloud it is under one fp32 spacing for about one query in 10^4.  (Members of one
    cluster have the same neighbours, so their features stay close and the clusters apart at the deeper levels as well.)"""
    n = M // k + (1 if M % k else 0)
    g = torch.Generator().manual_seed(seed)
    centre = synth_cloud(n, seed + 1)[0]
    member = torch.arange(M) // k
    pts = centre[member] + spread * (torch.rand(M, 6, generator=g) * 2 - 1)
    pd = ranking(pts[None])[0]
    full = member < M // k                                          # (the left-over points' k-th neighbour lies in another cluster)
    top = pd[full].sort(-1, descending=True).values
    assert float((top[:, k - 1] - top[:, k]).min()) > 1000 * fp32_dot_tol(pts[None]), "clusters too close"
    return pts[torch.randperm(M, generator=g)][None].contiguous()


def duplicates_cloud(n_distinct, copies, seed):
    """n_distinct points, each `copies` times, shuffled -> (pts [1, n_distinct * copies, 6], origin [M]: which distinct point a row is)."""
    base = synth_cloud(n_distinct, seed)
    perm = torch.randperm(n_distinct * copies, generator=torch.Generator().manual_seed(seed + 1))
    origin = (torch.arange(n_distinct * copies) % n_distinct)[perm]
    return base[:, origin].contiguous(), origin


def copies_agree(rows, origin):
    """rows [M, E]: True where all copies of every distinct point hold the same bits."""
    order = origin.sort(stable=True).indices
    n = int(origin.max()) + 1
    r = rows[order].reshape(n, -1, rows.shape[-1])
    return torch.equal(r, r[:, :1].expand_as(r))


def make_embedder(seed=7, n_neighbors=40):
    """modules.DGCNNembedder with the shipped head (six hidden layers of 512, 64 outputs) under a fixed seed, in eval mode, with every
    BatchNorm's affine parameters and running statistics randomised and every seventh BatchNorm weight NEGATIVE: the engine folds the
    scale s = weight / sqrt(var + eps) into the convolution BEFORE the max over neighbours (csrc/dgcnn_engine.cpp), which must hold for
    either sign of s."""
    from flowcompare_amd import modules
    torch.manual_seed(seed)
    emb = modules.DGCNNembedder(out_mlp_dims=[512] * 6, emb_dim=64, n_neighbors=n_neighbors)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for bn in (emb.bn1, emb.bn2, emb.bn3, emb.bn4, emb.bn5):
            n = bn.num_features
            w = 0.5 + torch.rand(n, generator=g)
            w[3::7] *= -1.0
            bn.weight.copy_(w)
            bn.bias.copy_(0.2 * torch.randn(n, generator=g))
            bn.running_mean.copy_(0.2 * torch.randn(n, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(n, generator=g))
    return emb.eval()


def embedder_state(emb, dtype=torch.float64):
    return {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in emb.state_dict().items()}


EMBED_CFG = {"input_embedder": "DGCNNembedder", "n_neighbors": 40}
