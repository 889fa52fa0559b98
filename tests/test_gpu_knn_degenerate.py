"""The DGCNN k-NN graph (csrc/knn.hip) where clouds are not in general position: lattices, exact duplicates, coincident points, fewer than
k distinct points, vanishing norms -- what voxelised coordinates and quantised colours produce.  Reference: tests/knn_ref_util.py (fp64,
the kernels' documented tie rule: lowest index among equal ranking values), checked on the host by tests/test_knn_ref_host.py.

1. integer clouds, where fp32 is exact: the set of every query EQUALS the stable fp64 top-k, for both kernels, cold and from every warm start
   (the cold result, the sets of a nearby feature space, and in place as the engine does between its levels);
2. clouds where rounding decides: valid sets within the fp32 dot-product bound, warm start bit-equal to cold, a scene's sets independent
   of its batch, refusals that launch nothing;
3. the embedder on a cloud of duplicates against the fp64 oracle; copies of a point get the same bits; warm start off == on; reversal."""
import ctypes

import pytest
import torch

import knn_ref_util as KU
from flowcompare_amd import engine
from knob_util import knobs
from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNELS = {"mfma-kernel": 2, "lane-per-candidate-kernel": 0}     # knob 24 (csrc/knobs.h)


@pytest.fixture(params=list(KERNELS.values()), ids=list(KERNELS))
def knn_kernel(request):
    with knobs({24: request.param}):
        yield request.param


def _sorted(idx):
    return idx.cpu().long().sort(-1).values


def _report(got, ref, what):
    bad = (got != ref).any(-1)
    if not bad.any():
        return ""
    b, i = (int(v) for v in bad.nonzero()[0])
    self_only = int((got == torch.arange(got.shape[1])[None, :, None]).all(-1).sum())
    return (f"{what}: {int(bad.sum())} of {bad.numel()} sets differ from the stable fp64 top-k ({self_only} queries returned k copies of themselves); "
            f"first: scene {b} query {i} got {got[b, i].tolist()} expected {ref[b, i].tolist()}")


# ------------------------------------------------------------------------------------------------ 1. exact set equality
@pytest.mark.parametrize("name,k", KU.EXACT_CASES, ids=[f"{n}-k{k}" for n, k in KU.EXACT_CASES])
def test_exact_cloud_sets_equal_the_stable_fp64_topk(name, k, knn_kernel):
    f = KU.exact_clouds()[name]
    got, ref = _sorted(engine.op_knn(f.to(DEV), k)), KU.exact_sets(name, k)
    assert torch.equal(got, ref), _report(got, ref, f"{name}, k = {k}, cold")


WARM_STARTS = ("its own cold result", "sets of the cloud with channel 0 doubled", "its own cold result, in place")


@pytest.mark.parametrize("warm_from", WARM_STARTS)
@pytest.mark.parametrize("name,k", KU.EXACT_CASES, ids=[f"{n}-k{k}" for n, k in KU.EXACT_CASES])
def test_exact_cloud_sets_from_a_warm_start(name, k, warm_from):
    f = KU.exact_clouds()[name].to(DEV)
    ref = KU.exact_sets(name, k)
    with knobs({24: 2, 32: 1}):
        if warm_from == WARM_STARTS[1]:
            warm = KU.exact_sets(name, k, doubled_channel=0).int()
        else:
            warm = engine.op_knn(f, k)
        keep = warm.clone()
        got = _sorted(engine.op_knn(f, k, warm=warm.to(DEV), in_place=warm_from == WARM_STARTS[2]))
    assert torch.equal(warm, keep)                                  # (in place works on a copy of its own)
    assert torch.equal(got, ref), _report(got, ref, f"{name}, k = {k}, warm start from {warm_from}")


# ------------------------------------------------------------------------------------------------ 2. where rounding decides
def _offset(B, M, C, seed):
    g = torch.Generator().manual_seed(seed)
    f = 30.0 + 0.01 * torch.randn(B, M, C, generator=g)
    return f, f + 0.003 * torch.randn(B, M, C, generator=g)


@pytest.mark.parametrize("B,M,C", [(1, 1024, 64), (2, 300, 6)])
def test_offset_cloud_sets_are_valid_and_warm_equals_cold(B, M, C):
    """f = 30 + 0.01 randn: |x|^2 ~ 900 C, neighbour gaps ~ 1e-4 C -- fp32 rounding of the ranking value (ulp(1800 C)) exceeds the gaps, so
    the two ways the matrix-core kernel computes it (the scalar chain of the warm start, the MFMA sums of the stream) really disagree and the
    warm-start threshold lives on its rounding bound alone."""
    k = 40
    f, near = _offset(B, M, C, 61)
    tol = KU.fp32_dot_tol(f)
    for name, knob in KERNELS.items():
        with knobs({24: knob}):
            idx = engine.op_knn(f.to(DEV), k).cpu()
        short = KU.check_sets(idx, f, k, tol)
        exact = (_sorted(idx) == KU.stable_topk(f, k)).all(-1).float().mean().item()
        print(f"offset cloud {B} x {M} x {C}, {name}: worst neighbour {short:.3e} below the fp64 k-th best (tolerance {tol:.3e}); "
              f"{100 * exact:.1f} % of the sets equal the fp64 top-{k}")
    with knobs({24: 2, 32: 1}):
        cold = engine.op_knn(f.to(DEV), k)
        for what, warm in (("its own result", cold), ("neighbours of f + 0.003 randn", engine.op_knn(near.to(DEV), k))):
            for in_place in (False, True):
                got = engine.op_knn(f.to(DEV), k, warm=warm, in_place=in_place)
                n = int((_sorted(got) != _sorted(cold)).any(-1).sum())
                assert n == 0, f"warm start from {what}{' in place' if in_place else ''}: {n} of {B * M} sets differ from the cold search"


@pytest.mark.parametrize("name", ["intfeat64", "lattice6"])
def test_tiny_cloud_sets_are_valid_and_warm_equals_cold(name, knn_kernel):
    """Features of norm ~2^-70: squares and products are subnormal or zero, every ranking value is a few subnormal steps from zero and the
    warm start's rounding bound underflows.  No reference ranks such a cloud to the bit; the sets must still be k distinct points, and the
    same with and without a warm start."""
    k = 40
    f = KU.exact_clouds()[name] * 2.0 ** -72
    assert float(f.abs().max()) > 0
    cold = engine.op_knn(f.to(DEV), k)
    KU.check_sets(cold.cpu(), f, k, None)
    if knn_kernel == 2:
        with knobs({32: 1}):
            for what, warm in (("its own result", cold), ("the unscaled cloud's sets", KU.exact_sets(name, k).int().to(DEV))):
                for in_place in (False, True):
                    got = engine.op_knn(f.to(DEV), k, warm=warm, in_place=in_place)
                    n = int((_sorted(got) != _sorted(cold)).any(-1).sum())
                    self_only = int((got.cpu() == torch.arange(f.shape[1])[None, :, None]).all(-1).sum())
                    assert n == 0, (f"warm start from {what}{' in place' if in_place else ''}: {n} of {cold.shape[0] * cold.shape[1]} sets differ "
                                    f"from the cold search ({self_only} queries returned k copies of themselves)")


def _quantised(B, M, C, seed, steps):
    """Features on a grid of 1 / steps in [-1, 1] (quantised colours, voxel centres): fp32-exact arithmetic, so plenty of exact ties."""
    g = torch.Generator().manual_seed(seed)
    return torch.round((torch.rand(B, M, C, generator=g) * 2 - 1) * steps) / steps


@pytest.mark.parametrize("B,M,C,knob24", [(3, 300, 64, 0), (16, 1024, 6, None), (2, 2085, 64, None)])
def test_a_scenes_sets_do_not_depend_on_its_batch(B, M, C, knob24):
    """csrc/knn.hip picks its kernel by M alone so that a scene's sets, ties and near-ties included, are the same alone and in any batch:
    one shape on each side of the M = 2048 boundary on the shipped knob, the lane kernel forced; quantised features at C = 6 (exact
    ties), continuous ones at C = 64 (near-ties)."""
    k = 40
    f = (_quantised(B, M, C, 71, 8) if C == 6 else torch.rand(B, M, C, generator=torch.Generator().manual_seed(71)) * 2 - 1).to(DEV)
    with knobs({} if knob24 is None else {24: knob24}):
        batch = engine.op_knn(f, k)
        KU.check_sets(batch[:2].cpu(), f[:2].cpu(), k, KU.fp32_dot_tol(f.cpu()))
        for b in range(B):
            assert torch.equal(engine.op_knn(f[b:b + 1], k), batch[b:b + 1]), f"scene {b} alone differs from its sets in the batch of {B}"
        if M >= 2048:                                               # the matrix-core kernel: the same from a warm start
            g = torch.Generator().manual_seed(72)
            warm = engine.op_knn(f + 0.1 * torch.randn(B, M, C, generator=g).to(DEV), k)
            wb = engine.op_knn(f, k, warm=warm)
            assert torch.equal(_sorted(wb), _sorted(batch))
            for b in range(B):
                assert torch.equal(engine.op_knn(f[b:b + 1], k, warm=warm[b:b + 1]), wb[b:b + 1]), f"warm start: scene {b} alone differs"
                assert torch.equal(engine.op_knn(f[b:b + 1], k, warm=warm[b:b + 1], in_place=True), wb[b:b + 1])


SENTINEL = -77


@pytest.mark.parametrize("B,M,C,k,code,why", [
    (1, 128, 6, 65, 6, "k beyond the 64 list entries"), (1, 128, 6, 0, 6, "k = 0"), (2, 30, 6, 40, 1, "fewer points than neighbours"),
    (1, 64, 512, 40, 6, "C over the lane kernel's LDS tile"), (1, 64, 457, 40, 6, "the first C over the tile (round_up(C, 4) = 460)"),
])
def test_refusals_return_their_status_and_launch_nothing(B, M, C, k, code, why, knn_kernel):
    f = torch.zeros(B, M, C, device=DEV)
    kk = max(k, 1)
    idx = torch.full((B, M, kk), SENTINEL, dtype=torch.int32, device=DEV)
    warm = torch.arange(kk, dtype=torch.int32, device=DEV).expand(B, M, kk).contiguous() % M
    L = engine.lib()
    engine.profile_stride(1); engine.profile_filter(None); engine.profile_enable(True); engine.profile_reset()
    try:
        with pytest.raises(engine.FcError) as e0:
            L.fc_op_knn_f32(engine._ptr(f), engine._ptr(idx), B, M, C, k, engine._stream())
        with pytest.raises(engine.FcError) as e1:
            L.fc_op_knn_warm_f32(engine._ptr(f), engine._ptr(warm), engine._ptr(idx), B, M, C, k, engine._stream())
        torch.cuda.synchronize()
        launched = [r["kernel"] for r in engine.profile_report()]
    finally:
        engine.profile_enable(False); engine.profile_reset()
    assert (e0.value.code, e1.value.code) == (code, code), why
    assert launched == [], f"{why}: a refused search launched {launched}"
    assert bool((idx == SENTINEL).all()), f"{why}: a refused search wrote to its output"


def test_widest_features_the_lane_kernel_accepts():
    """C = 456 fills the lane kernel's 160 KB of LDS to 192 bytes (csrc/knn.hip: knn_lane_lds); one more float4 of channels is refused above."""
    f = torch.rand(1, 70, 456, generator=torch.Generator().manual_seed(81)) * 2 - 1
    for knob in KERNELS.values():                                   # (C > 128: both settings take the lane kernel)
        with knobs({24: knob}):
            idx = engine.op_knn(f.to(DEV), 40).cpu()
        KU.check_sets(idx, f, 40, KU.fp32_dot_tol(f))
        assert (idx.long() == torch.arange(70)[None, :, None]).any(-1).all()


# ------------------------------------------------------------------------------------------------ 3. the embedder
Q99_GATE, MAX_GATE = 2e-5, 5e-3         # the gates of tests/test_gpu_configs.py on this embedder: per-row max |hip - fp64|


@pytest.fixture(scope="module")
def embedder():
    return KU.make_embedder().to(DEV)


@pytest.fixture(scope="module")
def embedder_sd(embedder):
    return KU.embedder_state(embedder)


def _embed(embedder, pts):
    with torch.no_grad():
        return embedder(pts.to(DEV)).cpu()


@pytest.mark.parametrize("n_distinct,copies", [(512, 4), (128, 4)], ids=["2048-points-mfma-kernel", "512-points-lane-kernel"])
def test_embedder_on_a_cloud_of_duplicates(embedder, embedder_sd, n_distinct, copies):
    """Every point four times, shuffled.  Ties exist only among copies of one point, which carry identical features, so any valid tie-break
    gives the same max over the neighbours (tests/test_knn_ref_host.py) and the fp64 oracle is a valid reference.  M = 2048 takes the
    matrix-core kernel and the in-place warm start of levels 1-3, M = 512 the lane kernel."""
    pts, origin = KU.duplicates_cloud(n_distinct, copies, 31)
    emb = _embed(embedder, pts)
    assert emb.shape == (1, n_distinct * copies, 64) and torch.isfinite(emb).all()
    with torch.no_grad():
        ref = O.dgcnn_embed(KU.EMBED_CFG, embedder_sd, pts.double())
    d = (emb.double() - ref).abs().amax(-1)[0]
    print(f"embedder, {n_distinct} points x {copies}: per-row max |hip - fp64| median {d.median():.2e} q99 {d.quantile(0.99):.2e} max {d.max():.2e} "
          f"(|embedding| max {float(ref.abs().max()):.2f})")
    assert d.quantile(0.99).item() < Q99_GATE and d.max().item() < MAX_GATE
    # copies of a point get the same bits
    assert KU.copies_agree(emb[0], origin), "copies of one point got different embeddings"
    # warm start off == on
    with knobs({32: 0}):
        assert torch.equal(_embed(embedder, pts), emb), "knob 32 = 0 (no warm start) changes the embedding"


@pytest.mark.parametrize("M", [2085, 300], ids=["2085-points-mfma-kernel", "300-points-lane-kernel"])
def test_embedder_commutes_with_reversal_and_ignores_the_warm_start(embedder, M):
    """A point's embedding must not depend on where it sits in the candidate stream or in a workgroup: M = 2085 is no multiple of 32, 64 or
    128 (partial tile, block and workgroup).  That holds for a cloud WITHOUT ties only -- "lowest index wins" names another winner once
    the stream is reversed -- and a uniform random cloud is not one: measured on the synth_pairs-style cloud below, 8 of 2085 rows
    (1 of 300) change under reversal, each of them a query whose 40th and 41st candidate at level 4 (128 channels, |x|^2 ~ 5, values
    0.1 .. 3.5 fp32 spacings apart in fp64) get the SAME fp32 ranking value; for the lane kernel the host emulation of its fmaf chains
    gives -0.05641079 for both.  So the equality is asserted on KU.clustered_cloud, random as well, whose k-th and (k + 1)-th
    neighbours are an inter-cluster distance apart; the uniform cloud keeps the warm-start clause and reports its count."""
    uniform = KU.synth_cloud(M, 41)
    emb = _embed(embedder, uniform)
    assert torch.isfinite(emb).all()
    with knobs({32: 0}):
        assert torch.equal(_embed(embedder, uniform), emb), "knob 32 = 0 (no warm start) changes the embedding"
    n = int((_embed(embedder, uniform.flip(1)).flip(1) != emb).any(-1).sum())
    print(f"uniform cloud, {M} points: {n} rows change under reversal (exact fp32 ties at the k-th neighbour)")
    pts = KU.clustered_cloud(M, 43)
    emb = _embed(embedder, pts)
    assert torch.isfinite(emb).all() and float(emb[0].std(0).max()) > 1e-4        # (the clusters do get different embeddings)
    with knobs({32: 0}):
        assert torch.equal(_embed(embedder, pts), emb), "knob 32 = 0 (no warm start) changes the embedding"
    rev = _embed(embedder, pts.flip(1)).flip(1)
    n = int((rev != emb).any(-1).sum())
    assert n == 0, f"{n} of {M} rows change when the cloud is reversed (max difference {float((rev - emb).abs().max()):.2e})"
