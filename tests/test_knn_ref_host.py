"""The reference of the degenerate-cloud k-NN tests (tests/knn_ref_util.py) checked on the host: the stable top-k against a plain loop, the
lattice really separates the documented tie rule from torch.topk's, and the two properties of the fp64 oracle that let it judge the HIP
embedder on a cloud full of duplicates although its own tie order is arbitrary.  Runs on the CPU."""
import torch

import knn_ref_util as KU
from oracle import flow_oracle as O


def test_stable_topk_matches_a_plain_loop():
    ax = torch.arange(-1, 2).float()
    lattice = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(27, 3)
    few = KU._ints(1, 8, 4, -1, 1).repeat(3, 1)                      # 8 distinct rows three times: ties of every query with itself
    for s0, k in ((lattice, 7), (lattice, 27), (few, 5), (few, 1)):
        f = torch.stack((s0, s0.flip(0)))
        got = KU.stable_topk(f, k)
        assert got.dtype == torch.int64 and got.shape == (2, s0.shape[0], k)
        assert torch.equal(got, KU.brute_topk(f, k))
    f = torch.randn(1, 30, 5, generator=torch.Generator().manual_seed(2))          # no ties: the plain top-k
    assert torch.equal(KU.stable_topk(f, 6), KU.ranking(f).topk(6, dim=-1).indices.sort(-1).values)


def test_exact_clouds_have_their_shapes_and_are_exact():
    shapes = {n: tuple(f.shape) for n, f in KU.exact_clouds().items()}
    assert shapes == {"lattice3": (2, 512, 3), "lattice6": (2, 512, 6), "intfeat64": (2, 300, 64), "intfeat100": (2, 129, 100),
                      "copies": (2, 320, 16), "zero_cluster": (2, 300, 64), "all_equal": (2, 128, 6), "all_zero": (2, 128, 6),
                      "m_eq_k_40": (2, 40, 6), "m_eq_k_64": (2, 64, 64), "tail2085": (2, 2085, 6)}
    cl = KU.exact_clouds()
    for name, f in cl.items():
        assert torch.equal(f[1], f[0].flip(0))
        # exactness, on the ranking itself: rounding it to fp32 changes nothing, and neither does forming it in fp32
        pd = KU.ranking(f)
        assert torch.equal(pd.float().double(), pd)
        f32 = 2 * (f @ f.transpose(1, 2)) - (f ** 2).sum(-1)[:, None, :] - (f ** 2).sum(-1)[:, :, None]
        assert torch.equal(f32.double(), pd), name
    assert (cl["lattice3"][0] == 0).all(-1).any()                   # the origin is a lattice point
    assert bool((cl["zero_cluster"][0, 100:170] == 0).all()) and int((cl["zero_cluster"][0] == 0).all(-1).sum()) == 70
    assert torch.unique(cl["copies"][0], dim=0).shape[0] == 80 and torch.equal(cl["copies"][0, :80], cl["copies"][0, 240:])
    assert KU.ks_of("lattice3") == [8, 40, 64] and KU.ks_of("m_eq_k_40") == [8, 40] and KU.ks_of("m_eq_k_64") == [8, 40, 64]
    for name, k in KU.EXACT_CASES[:6]:
        assert torch.equal(KU.exact_sets(name, k), KU.stable_topk(cl[name], k))
    assert not torch.equal(KU.exact_sets("lattice3", 40, 0), KU.exact_sets("lattice3", 40))       # the doubled axis is another space


def test_lattice_separates_the_stable_rule_from_torch_topk():
    f = KU.exact_clouds()["lattice3"]
    for k in (8, 40):
        stable = KU.exact_sets("lattice3", k)
        plain = KU.ranking(f).topk(k, dim=-1).indices.sort(-1).values
        differ = int((stable != plain).any(-1).sum())
        print(f"lattice3, k = {k}: torch.topk's set differs from the lowest-index-first set for {differ} of {stable.shape[0] * stable.shape[1]} queries")
        assert differ > 0
        # both are valid top-k sets: the same ranking values
        pd = KU.ranking(f)
        assert torch.equal(torch.gather(pd, 2, stable).sort(-1).values, torch.gather(pd, 2, plain).sort(-1).values)


def test_clustered_cloud_has_no_near_ties_where_the_uniform_cloud_has():
    """The reversal test needs a cloud without ties at the k-th neighbour.  In the uniform cloud some query's 40th and 41st candidate are
    closer than the fp32 error of a ranking value already at level 1; in the clustered cloud the members of full clusters keep 1000 x that."""
    for M in (2085, 300):
        pts = KU.clustered_cloud(M, 43)
        assert pts.shape == (1, M, 6) and torch.unique(pts[0], dim=0).shape[0] == M
        top = KU.ranking(pts)[0].sort(-1, descending=True).values
        gap = top[:, 39] - top[:, 40]
        tol = KU.fp32_dot_tol(pts)
        assert int((gap > 1000 * tol).sum()) >= M // 40 * 40 and float(gap.min()) > tol
    uni = KU.synth_cloud(2085, 41)
    top = KU.ranking(uni)[0].sort(-1, descending=True).values
    assert float((top[:, 39] - top[:, 40]).min()) < KU.fp32_dot_tol(uni)


def test_fp64_trunk_gives_copies_the_same_bits_and_commutes_with_permutations():
    """Ties of the duplicates cloud are ties among copies of one point, which carry identical features at every level: whichever of them
    torch.topk keeps, the max over the neighbours is the same.  So the oracle's rows for the copies of a point agree bit for bit, and so do
    the rows of one point under a permutation of the cloud -- which makes the oracle a valid reference for the HIP embedder there."""
    sd = KU.embedder_state(KU.make_embedder())
    pts, origin = KU.duplicates_cloud(512, 4, 31)
    assert pts.shape == (1, 2048, 6) and torch.equal(pts[0, origin == 5][0], pts[0, origin == 5][3])
    with torch.no_grad():
        t = O.dgcnn_trunk(sd, pts.double(), 40)
        perm = torch.randperm(2048, generator=torch.Generator().manual_seed(3))
        tp = O.dgcnn_trunk(sd, pts[:, perm].double(), 40)
    assert torch.isfinite(t).all() and float(t.abs().max()) > 0
    assert KU.copies_agree(t[0], origin)
    assert torch.equal(tp[0], t[0, perm])
    neg = [int((sd[f"bn{i}.weight"] < 0).sum()) for i in range(1, 6)]
    assert all(n >= 9 for n in neg), neg                            # the sign of the BatchNorm scale is part of what the GPU tests pin
