"""Scene staging that keeps voxels with sparse context (include/fcflow_sparse_stage.h, csrc/scene_stage.hip) on the
GPU: the ragged FPS with a sample count per voxel and the pair kernel against the existing single-pair API (staging.fps / staging.stage_pair),
stage_scene(min_context) against the numpy restatement of tests/sparse_stage_util.py, and scene_change / dense_log_prob /
scene_context_attribution with min_context against their hand-written compositions.  The scene is the fixture scene with the roles swapped:
context = the thinned cloud, whose 32 context boxes hold 400 .. 1486 points (pinned in tests/test_sparse_stage_host.py), M = 1280, N = 64."""
import contextlib
import io

import numpy as np
import pytest
import torch

import flowcompare_amd as fa
import scene_stage_util as U
import sparse_stage_util as SU
from flowcompare_amd import change, engine, staging

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, N = SU.M, SU.N


@pytest.fixture(scope="module")
def scene():
    c0, c1 = SU.swapped_scene()
    return torch.from_numpy(c0).to(DEV), torch.from_numpy(c1).to(DEV), torch.from_numpy(U.centers_np()).to(DEV)


@pytest.fixture(scope="module")
def staged(scene):
    c0, c1, centers = scene
    return staging.stage_scene(c0, c1, centers, U.FINAL, U.CONTEXT, N, M, ground_height=U.GROUND, min_context=256)


def _model(**kw):
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=2, sample_size=N, n_samples_context=M, **kw)
    cfg["final_voxel_size"], cfg["context_voxel_size"] = U.FINAL, U.CONTEXT
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    return cfg, md


@pytest.fixture(scope="module")
def model():
    return _model()


def _fps_crop(voxel, m):
    """the existing API on one cropped voxel: its picks for m samples"""
    return staging.fps(voxel, torch.zeros(voxel.shape[0], dtype=torch.long, device=voxel.device), ratio=m / voxel.shape[0], random_start=False)[:m]


def _same(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(-1.0), b.nan_to_num(-1.0))


def _check_fps_counts(cloud, off, rows, m, voxel_ids=None):
    """fps_ragged_counts on (off, rows[, voxel_ids]) against staging.fps on every crop; returns (idx, counts)."""
    idx, cnt = staging.fps_ragged_counts(cloud, off, rows, m, voxel_ids)
    ids = list(range(off.numel() - 1)) if voxel_ids is None else voxel_ids.tolist()
    assert idx.shape == (len(ids), m) and idx.dtype == torch.int64 and cnt.shape == (len(ids),) and cnt.dtype == torch.int32
    sizes = [int(off[v + 1] - off[v]) for v in ids]
    assert cnt.tolist() == [min(n, m) for n in sizes]
    for i, (v, n) in enumerate(zip(ids, sizes)):
        mv = min(n, m)
        assert bool((idx[i, mv:] == -1).all()), (i, n)
        if mv:
            mem = rows[off[v]:off[v + 1]].long()
            assert torch.equal(idx[i, :mv], mem[_fps_crop(cloud[mem], mv)]), (i, n, m)
    idx2, cnt2 = staging.fps_ragged_counts(cloud, off, rows, m, voxel_ids)
    assert torch.equal(idx, idx2) and torch.equal(cnt, cnt2)                      # same input, same bytes
    return idx, cnt


def _csr(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=DEV)


# ---------------------------------------------------------------- 1. ragged FPS with a sample count per voxel
def test_fps_counts_on_the_fixture_lists(scene):
    c0, _, centers = scene
    off, rows = staging.voxel_rows(c0, centers, U.CONTEXT)
    sizes = (off[1:] - off[:-1]).tolist()
    assert min(sizes) == 400 and max(sizes) == 1486 and sum(n < M for n in sizes) == 20
    idx, cnt = _check_fps_counts(c0, off, rows, M)
    # the existing entry on the same lists with m <= the smallest voxel: unchanged, and a prefix of the longer selections
    old = staging.fps_ragged(c0, off, rows, 400)
    assert torch.equal(old, idx[:, :400])
    for k in (0, 31, sizes.index(400)):
        mem = rows[off[k]:off[k + 1]]
        assert torch.equal(old[k], mem[_fps_crop(c0[mem], 400)]), k
    with pytest.raises(RuntimeError, match="fps_ragged"):
        staging.fps_ragged(c0, off, rows, 401)


def test_fps_counts_on_hand_made_lists():
    m = 50
    g = torch.Generator().manual_seed(4)
    sizes = [1, m - 1, 0, m, m + 1]                                               # n = 1, m - 1, an empty voxel, m, m + 1
    cloud = torch.rand(sum(sizes), 6, generator=g).to(DEV)
    idx, cnt = _check_fps_counts(cloud, _csr(sizes), torch.arange(cloud.shape[0], device=DEV), m)
    assert cnt.tolist() == [1, m - 1, 0, m, m] and bool((idx[2] == -1).all()) and int(idx[0, 0]) == 0
    assert sorted(idx[1, :m - 1].tolist()) == list(range(1, m))                   # n < m: a permutation of the voxel
    # a tie lattice (the 8 x 8 grid of test_fps_ragged_equals_fps_on_every_cropped_voxel): m above, at and below the voxels' sizes
    grid = torch.stack(torch.meshgrid(torch.arange(8.0), torch.arange(8.0), indexing="ij"), -1).reshape(-1, 2)
    parts = [grid[:64], grid[:40] + 100, grid[:17] * 2 - 50, grid[:64].flip(0) + 7]
    lattice = torch.cat(parts).to(DEV).contiguous()
    off = _csr([p.shape[0] for p in parts])
    rows = torch.arange(lattice.shape[0], device=DEV)
    for mm in (1, 17, 40, 64, 70):
        _check_fps_counts(lattice, off, rows, mm)
    # rows that are not contiguous, voxels that overlap, voxel_ids out of order and repeated
    perm = torch.randperm(lattice.shape[0], generator=torch.Generator().manual_seed(5)).to(DEV)
    lists = [perm[:50].sort().values, perm[20:120].sort().values, perm[100:103].sort().values]
    idx, cnt = _check_fps_counts(lattice, _csr([50, 100, 3]), torch.cat(lists), 60, torch.tensor([1, 2, 0, 1], device=DEV))
    assert cnt.tolist() == [60, 3, 50, 60] and torch.equal(idx[0], idx[3])
    # every listed voxel sparse: m above the largest voxel
    small = torch.rand(23, 3, generator=g).to(DEV)
    idx, cnt = _check_fps_counts(small, _csr([5, 17, 1]), torch.arange(23, device=DEV), 32)
    assert cnt.tolist() == [5, 17, 1]
    with pytest.raises(RuntimeError, match="samples asked"):
        staging.fps_ragged_counts(small, _csr([5, 17, 1]), torch.arange(23, device=DEV), 0)
    with pytest.raises(RuntimeError, match="voxel_ids"):
        staging.fps_ragged_counts(small, _csr([5, 17, 1]), torch.arange(23, device=DEV), 4, torch.tensor([3], device=DEV))


def test_fps_counts_with_a_voxel_on_the_global_scratch_path():
    """30 000 rows (running distances in global scratch, m_v = m) between a sparse voxel and an LDS-resident one, in one launch."""
    big = torch.rand(33020, 6, generator=torch.Generator().manual_seed(9)).to(DEV)
    idx, cnt = _check_fps_counts(big, _csr([20, 30000, 3000]), torch.arange(33020, device=DEV), 48)
    assert cnt.tolist() == [20, 48, 48]


# ---------------------------------------------------------------- 2. the pair kernel and stage_scene(min_context)
def test_stage_scene_with_min_context_equals_stage_pair_per_voxel(scene, staged):
    c0, c1, centers = scene
    st = staged
    o0, r0 = staging.voxel_rows(c0, centers, U.CONTEXT)
    o1, r1 = staging.voxel_rows(c1, centers, U.FINAL)
    assert st.voxel.tolist() == list(range(32)) and st.context_counts.dtype == torch.int32 and st.context_counts.is_cuda
    assert torch.equal(st.context_counts, st.count_0.clamp(max=M)) and st.extract_0.shape == (32, M, 6) and st.index_0.shape == (32, M)
    counts = st.context_counts.tolist()
    assert sum(c < M for c in counts) == 20 and min(counts) == 400
    for k, c in enumerate(counts):
        v0, v1 = c0[r0[o0[k]:o0[k + 1]]], c1[r1[o1[k]:o1[k + 1]]]
        s0, s1, inv = staging.stage_pair(v0, v1, c, N)
        assert torch.equal(st.extract_0[k, :c], s0) and torch.equal(st.extract_1[k], s1), (k, c)
        assert torch.equal(st.inverse["furthest_distance"][k], inv["furthest_distance"]) and torch.equal(st.inverse["mean"][k], inv["mean"]), k
        assert torch.equal(st.extra_context[k], (inv["mean"][2] - U.GROUND).unsqueeze(-1))
        assert bool((st.extract_0[k, c:] == 0).all()) and bool((st.index_0[k, c:] == -1).all()) and bool((st.index_0[k, :c] >= 0).all()), k
        assert torch.equal(c0[st.index_0[k, :c]][:, 3:], st.extract_0[k, :c, 3:])
    # inner_loop's own check of the counts accepts them
    assert engine._context_counts(st.context_counts, 32, M, DEV) is not None
    # the pair kernel on its own: counts outside [1, M] are clamped, never an out-of-range read; full counts equal co_unit_sphere
    full = torch.full((32,), M + 5, dtype=torch.int32, device=DEV)
    heavy = torch.nonzero(st.count_0 >= M).flatten()
    a0, a1, ainv = engine.stage_pairs_counts(c0, c1, st.index_0[heavy].contiguous(), st.index_1[heavy].contiguous(), full[:heavy.numel()].contiguous())
    b0, b1, binv = engine.stage_co_unit_sphere(c0[st.index_0[heavy]], c1[st.index_1[heavy]])
    assert heavy.numel() == 12 and torch.equal(a0, b0) and torch.equal(a1, b1) and torch.equal(ainv, binv)
    z0, _, _ = engine.stage_pairs_counts(c0, c1, st.index_0[:2].contiguous(), st.index_1[:2].contiguous(), torch.zeros(2, dtype=torch.int32, device=DEV))
    assert bool((z0[:, 1:] == 0).all()) and bool(torch.isfinite(z0).all())


def _assert_fp64_tie(a, b, cloud, what):
    """test_gpu_scene_stage's rule: a selection may differ from the restatement only where, at the first differing pick, both candidates'
    running distances (fp64, to the picks before it) tie within 1e-6 relative."""
    d = np.nonzero(a != b)[0]
    if len(d) == 0:
        return
    j = d[0]
    prev = cloud[a[:j]].astype(np.float64)
    da, db = (((cloud[p].astype(np.float64) - prev) ** 2).sum(-1).min() for p in (a[j], b[j]))
    print(f"{what}: first differing pick {j}: running distances {da!r} vs {db!r}")
    assert abs(da - db) <= 1e-6 * max(da, db)


def test_stage_scene_with_min_context_against_the_numpy_restatement(staged):
    st = staged
    n0, n1 = SU.swapped_scene()
    r = SU.stage_sparse_np(n0, n1, U.centers_np(), U.FINAL, U.CONTEXT, N, M, 256)
    assert st.voxel.tolist() == r["voxel"].tolist() and st.context_counts.tolist() == r["context_counts"].tolist()
    assert np.array_equal(st.count_0.cpu().numpy(), r["count_0"]) and np.array_equal(st.count_1.cpu().numpy(), r["count_1"])
    skipped = 0
    for i in range(32):
        i0, i1 = st.index_0[i].cpu().numpy(), st.index_1[i].cpu().numpy()
        if not (np.array_equal(i0, r["index_0"][i]) and np.array_equal(i1, r["index_1"][i])):
            c = int(r["context_counts"][i])
            _assert_fp64_tie(i0[:c], r["index_0"][i][:c], n0, f"voxel {i} index_0")
            _assert_fp64_tie(i1, r["index_1"][i], n1, f"voxel {i} index_1")
            skipped += 1
            continue
        e0 = np.abs(st.extract_0[i].cpu().numpy() - r["extract_0"][i]).max()
        e1 = np.abs(st.extract_1[i].cpu().numpy() - r["extract_1"][i]).max()
        assert e0 < 1e-6 and e1 < 1e-6, (i, e0, e1)
        assert abs(float(st.inverse["furthest_distance"][i]) - float(r["far"][i])) < 1e-4
        assert np.abs(st.inverse["mean"][i].cpu().numpy() - r["mean"][i]).max() < 1e-5
    print(f"voxels whose selection differs from the numpy restatement at an fp64 tie: {skipped}")
    assert skipped <= 1


def test_min_context_values(scene, staged, monkeypatch):
    c0, c1, centers = scene
    args = (c0, c1, centers, U.FINAL, U.CONTEXT, N, M)
    fields = ("extract_0", "extract_1", "extra_context", "index_0", "index_1", "voxel", "count_0", "count_1")

    def same(a, b):
        return all(torch.equal(getattr(a, f), getattr(b, f)) for f in fields) and all(torch.equal(a.inverse[k], b.inverse[k]) for k in a.inverse)

    today = staging.stage_scene(*args, ground_height=U.GROUND)
    none = staging.stage_scene(*args, ground_height=U.GROUND, min_context=None)
    assert same(today, none) and none.context_counts is None and today.voxel.numel() == 12
    at_m = staging.stage_scene(*args, ground_height=U.GROUND, min_context=M)
    assert same(today, at_m) and at_m.context_counts.tolist() == [M] * 12 and bool((at_m.index_0 >= 0).all())
    st512 = staging.stage_scene(*args, min_context=512)
    assert st512.voxel.numel() == 30 and st512.extra_context is None and int(st512.context_counts.min()) == 1064
    keep = torch.tensor([k in st512.voxel.tolist() for k in range(32)], device=DEV)
    assert torch.equal(st512.extract_0, staged.extract_0[keep]) and torch.equal(st512.index_0, staged.index_0[keep])
    assert torch.equal(st512.context_counts, staged.context_counts[keep])
    empty = staging.stage_scene(c0, c1, centers + 1000.0, U.FINAL, U.CONTEXT, N, M, min_context=256)
    assert empty.voxel.numel() == 0 and empty.context_counts.shape == (0,) and empty.context_counts.dtype == torch.int32

    def never(*a, **k):
        raise AssertionError("launched before the refusal")
    for name in ("stage_voxel_count", "stage_voxel_select", "stage_fps_ragged", "stage_fps_ragged_counts", "stage_pairs_counts", "stage_co_unit_sphere"):
        monkeypatch.setattr(engine, name, never)
    cfg, md = _model()
    for bad in (0, M + 1, 2.5, torch.tensor(256, device=DEV)):
        with pytest.raises(RuntimeError, match="min_context must"):
            staging.stage_scene(*args, min_context=bad)
        with pytest.raises(RuntimeError, match="scene_change: min_context must"):
            fa.scene_change(c0, c1, md, cfg, centers, ground_height=U.GROUND, min_context=bad)
        with pytest.raises(RuntimeError, match="scene_context_attribution: min_context must"):
            fa.scene_context_attribution(c0, c1, md, cfg, centers, ground_height=U.GROUND, min_context=bad)
    md["flow"].train()
    with pytest.raises(RuntimeError, match="scene_change: min_context is eval-mode only"):
        fa.scene_change(c0, c1, md, cfg, centers, ground_height=U.GROUND, min_context=256)


# ---------------------------------------------------------------- 3. scene_change, sampled and dense
KW = dict(ground_height=U.GROUND, multiple=1.0, voxels_per_batch=7)           # multiple = 1: some points of every voxel are marked


def _by_hand_stagings(scene):
    c0, c1, centers = scene
    ok = (staging.voxel_counts(c0, centers, U.CONTEXT) >= 256) & (staging.voxel_counts(c1, centers, U.FINAL) >= N) & \
        (staging.voxel_counts(c0, centers, U.FINAL) >= N)
    assert int(ok.sum()) == 32
    sel = centers[ok].contiguous()
    s10 = staging.stage_scene(c0, c1, sel, U.FINAL, U.CONTEXT, N, M, U.GROUND, min_context=256)
    s00 = staging.stage_scene(c0, c0, sel, U.FINAL, U.CONTEXT, N, M, U.GROUND, min_context=256)
    assert torch.equal(s10.context_counts, s00.context_counts) and torch.equal(s10.index_0, s00.index_0)
    return sel, s10, s00


def test_scene_change_with_min_context_equals_the_hand_written_composition(scene, model):
    c0, c1, centers = scene
    cfg, md = model
    torch.manual_seed(11)
    out, st = fa.scene_change(c0, c1, md, cfg, centers, min_context=256, **KW)
    torch.manual_seed(11)
    out_none, st_none = fa.scene_change(c0, c1, md, cfg, centers, **KW)
    assert st_none.context_counts is None and st_none.voxel.numel() == 12

    sel, s10, s00 = _by_hand_stagings(scene)
    torch.manual_seed(11)
    chunks = []
    for a in range(0, 32, 7):
        ex, cnt = s10.extra_context[a:a + 7], s10.context_counts[a:a + 7]
        _, l10, _ = fa.inner_loop((s10.extract_0[a:a + 7], s10.extract_1[a:a + 7], ex), md, cfg, context_counts=cnt)
        _, l00, _ = fa.inner_loop((s00.extract_0[a:a + 7], s00.extract_1[a:a + 7], ex), md, cfg, context_counts=cnt)
        chunks.append(change.log_prob_to_change(l10, l00, 1.0))
    ref = torch.full((c1.shape[0],), float("nan"), device=DEV)
    ref.scatter_reduce_(0, s10.index_1.reshape(-1), torch.cat(chunks).reshape(-1), "amax", include_self=False)
    assert _same(out, ref)
    touched = torch.zeros(c1.shape[0], dtype=torch.bool, device=DEV)
    touched[s10.index_1.reshape(-1)] = True
    assert torch.equal(torch.isfinite(out), touched) and torch.equal(out.isnan(), ~touched)
    assert float(out[touched].min()) >= 0.0 and float(out[touched].max()) <= 1.0 and bool((out[touched] > 0).any())
    assert torch.equal(st.index_1, s10.index_1) and torch.equal(st.context_counts, s10.context_counts) and st.voxel.tolist() == list(range(32))
    assert st.count_0.shape == (32,)
    # what it buys: strictly more points evaluated, none lost
    fin, fin_none = torch.isfinite(out), torch.isfinite(out_none)
    assert int(fin.sum()) > int(fin_none.sum()) > 0 and bool(fin[fin_none].all())
    print(f"sampled: {int(fin_none.sum())} points finite without min_context, {int(fin.sum())} with min_context = 256")


def test_a_sparse_voxel_in_a_chunk_scores_as_it_does_alone(scene, model):
    """Pinned eps: the chunk that holds a sparse voxel gives it, bit for bit, the log-prob of a one-voxel inner_loop on its truncated pair."""
    cfg, md = model
    _, s10, _ = _by_hand_stagings(scene)
    counts = s10.context_counts.tolist()
    sparse = [k for k, c in enumerate(counts) if c < 1000]
    assert [counts[k] for k in sparse] in ([400, 403], [403, 400])
    g = torch.Generator().manual_seed(3)
    for k in sparse + [next(k for k, c in enumerate(counts) if 1000 <= c < M)]:
        a, c = (k // 7) * 7, counts[k]
        b = min(a + 7, 32)
        eps = [torch.randn(s, generator=g).to(DEV) for s in md["flow"].noise_shapes(b - a, N)]
        batch = (s10.extract_0[a:b], s10.extract_1[a:b], s10.extra_context[a:b])
        _, lp, _ = fa.inner_loop(batch, md, cfg, eps=eps, context_counts=s10.context_counts[a:b])
        one = (s10.extract_0[k:k + 1, :c].contiguous(), s10.extract_1[k:k + 1], s10.extra_context[k:k + 1])
        _, alone, _ = fa.inner_loop(one, md, cfg, eps=[e[k - a:k - a + 1] for e in eps])
        d = (lp[k - a:k - a + 1] - alone).abs().max().item()
        print(f"voxel {k} ({c} context points) in its chunk of {b - a} against alone: max |d| {d:.2e}")
        assert bool(torch.isfinite(alone).all()) and torch.equal(lp[k - a:k - a + 1], alone), (k, c, d)


def test_dense_scene_change_with_min_context(scene, model):
    c0, c1, centers = scene
    cfg, md = model
    torch.manual_seed(11)
    out, st = fa.scene_change(c0, c1, md, cfg, centers, dense=True, block=256, min_context=256, **KW)
    torch.manual_seed(11)
    out_none, _ = fa.scene_change(c0, c1, md, cfg, centers, dense=True, block=256, **KW)

    sel, s10, s00 = _by_hand_stagings(scene)
    dense = staging.stage_dense(c1, s10, U.FINAL, sel, 256)
    torch.manual_seed(11)
    l10 = fa.dense_log_prob(s10, dense, md, cfg, blocks_per_batch=7)
    l00 = torch.cat([fa.inner_loop((s00.extract_0[a:a + 7], s00.extract_1[a:a + 7], s10.extra_context[a:a + 7]), md, cfg,
                                   context_counts=s10.context_counts[a:a + 7])[1] for a in range(0, 32, 7)])
    assert l10.shape == (dense.rows.numel(),) and l00.shape == (32, N)
    vals = change.log_prob_to_change_ragged(l10, dense.offsets, l00, 1.0)
    ref = torch.full((c1.shape[0],), float("nan"), device=DEV)
    ref.scatter_reduce_(0, dense.rows, vals, "amax", include_self=False)
    assert _same(out, ref)
    assert torch.equal(st.dense.index, dense.index) and torch.equal(st.context_counts, s10.context_counts)
    touched = torch.zeros(c1.shape[0], dtype=torch.bool, device=DEV)
    touched[dense.rows] = True
    assert torch.equal(torch.isfinite(out), touched) and torch.equal(out.isnan(), ~touched)
    assert float(out[touched].min()) >= 0.0 and float(out[touched].max()) <= 1.0 and bool((out[touched] > 0).any())
    fin, fin_none = torch.isfinite(out), torch.isfinite(out_none)
    assert int(fin.sum()) > int(fin_none.sum()) > 0 and bool(fin[fin_none].all())
    print(f"dense: {int(fin_none.sum())} points finite without min_context, {int(fin.sum())} with min_context = 256")

    # a sparse voxel's members, pinned eps: the whole-scene call against dense_log_prob of that voxel alone on its truncated context
    widths = [s[2] for s in md["flow"].noise_shapes(1, 1)]
    g = torch.Generator().manual_seed(5)
    eps = [torch.randn(dense.rows.numel(), w, generator=g).to(DEV) for w in widths]
    whole = fa.dense_log_prob(s10, dense, md, cfg, blocks_per_batch=7, eps=eps)
    counts = s10.context_counts.tolist()
    for k in [k for k, c in enumerate(counts) if c < 1000]:
        c = counts[k]
        s1 = staging.stage_scene(c0, c1, sel[k:k + 1].contiguous(), U.FINAL, U.CONTEXT, N, M, U.GROUND, min_context=256)
        d1 = staging.stage_dense(c1, s1, U.FINAL, sel[k:k + 1].contiguous(), 256)
        assert s1.context_counts.tolist() == [c] and torch.equal(s1.extract_0, s10.extract_0[k:k + 1])
        s1.extract_0, s1.context_counts = s1.extract_0[:, :c].contiguous(), None          # the truncated pair, through the path without counts
        lo, hi = int(dense.offsets[k]), int(dense.offsets[k + 1])
        assert torch.equal(d1.rows, dense.rows[lo:hi])
        alone = fa.dense_log_prob(s1, d1, md, cfg, blocks_per_batch=7, eps=[e[lo:hi] for e in eps])
        d = (whole[lo:hi] - alone).abs().max().item()
        print(f"dense voxel {k} ({c} context points, {hi - lo} members) in the scene against alone: max |d| {d:.2e}")
        assert torch.equal(whole[lo:hi], alone), (k, c, d)


# ---------------------------------------------------------------- 4. scene_context_attribution
def test_scene_context_attribution_with_min_context(scene):
    c0, c1, centers = scene
    cfg, md = _model(latent_dim=16, cif_latent_dim=16)
    layers = ["aug", 1]
    torch.manual_seed(11)
    mass_0, change_1, st = fa.scene_context_attribution(c0, c1, md, cfg, centers, layers=layers, min_context=256, **KW)
    assert tuple(mass_0.shape) == (2, c0.shape[0]) and tuple(change_1.shape) == (c1.shape[0],)

    sel, s10, s00 = _by_hand_stagings(scene)
    torch.manual_seed(11)
    chunks, masses = [], []
    for a in range(0, 32, 7):
        ex, cnt = s10.extra_context[a:a + 7], s10.context_counts[a:a + 7]
        b10 = (s10.extract_0[a:a + 7], s10.extract_1[a:a + 7], ex)
        eps = [torch.randn(s, device=DEV) for s in md["flow"].noise_shapes(b10[1].shape[0], N)]
        _, a10, _ = fa.inner_loop(b10, md, cfg, eps=eps, context_counts=cnt)
        _, a00, _ = fa.inner_loop((s00.extract_0[a:a + 7], s00.extract_1[a:a + 7], ex), md, cfg, eps=eps, context_counts=cnt)
        ch = change.log_prob_to_change(a10, a00, 1.0)
        chunks.append(ch)
        masses.append(torch.stack(fa.attention_mass(b10, md, cfg, layers=layers, weights=ch, eps=eps, context_counts=cnt)))
    ref_c = torch.full((c1.shape[0],), float("nan"), device=DEV)
    ref_c.scatter_reduce_(0, s10.index_1.reshape(-1), torch.cat(chunks).reshape(-1), "amax", include_self=False)
    flat = s10.index_0.reshape(-1)
    real = flat >= 0
    allm = torch.cat(masses, dim=1).reshape(2, -1)
    assert bool((allm[:, ~real] == 0).all())                                      # pad slots hold exact zeros ...
    ref_m = torch.full((2, c0.shape[0]), float("nan"), device=DEV)
    for i in range(2):
        ref_m[i].scatter_reduce_(0, flat[real], allm[i][real], "amax", include_self=False)
    assert _same(change_1, ref_c) and _same(mass_0, ref_m)
    touched = torch.zeros(c0.shape[0], dtype=torch.bool, device=DEV)
    touched[flat[real]] = True
    assert 0 < int(touched.sum()) < c0.shape[0] and int((~real).sum()) == int((M - s10.context_counts.long()).sum()) > 0
    for i in range(2):                                                            # ... and reach no row: finite exactly on the rows index_0 >= 0 names
        assert torch.equal(torch.isfinite(mass_0[i]), touched) and torch.equal(mass_0[i].isnan(), ~touched)
    assert torch.equal(st.index_0, s10.index_0) and torch.equal(st.context_counts, s10.context_counts)
    assert float(mass_0[:, touched].min()) >= 0.0 and bool((mass_0[:, touched] > 0).any())


def test_attribution_change_equals_scene_change_with_min_context(scene):
    """For a flow that draws no noise (latent_dim == input_dim) both are the same function of the seed."""
    c0, c1, centers = scene
    cfg, md = _model(latent_dim=6, cif_latent_dim=6)
    assert md["flow"].noise_shapes(7, N) == []
    torch.manual_seed(11)
    _, change_1, st = fa.scene_context_attribution(c0, c1, md, cfg, centers, layers="all", min_context=256, **KW)
    torch.manual_seed(11)
    ref, st_ref = fa.scene_change(c0, c1, md, cfg, centers, min_context=256, **KW)
    assert _same(change_1, ref) and int(torch.isfinite(ref).sum()) > 0
    assert torch.equal(st.index_0, st_ref.index_0) and st.voxel.tolist() == st_ref.voxel.tolist() == list(range(32))
