"""Staging of whole scene pairs on the GPU (csrc/scene_stage.hip through flowcompare_amd.staging / fa.scene_change) against the
reference's member lists (tests/golden/scene_stage_*.npz), the existing single-pair API (staging.fps / staging.stage_pair, themselves
pinned by tests/test_gpu_staging.py) and the numpy restatement of tests/scene_stage_util.py."""
import contextlib
import io
import statistics
import time

import numpy as np
import pytest
import torch

import flowcompare_amd as fa
import scene_stage_util as U
from flowcompare_amd import change, staging

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fx():
    return U.load_fixture()


@pytest.fixture(scope="module")
def scene():
    c0, c1 = U.scene()
    return torch.from_numpy(c0).to(DEV), torch.from_numpy(c1).to(DEV), torch.from_numpy(U.centers_np()).to(DEV)


def _fps_crop(voxel, m):
    """the parent API on one cropped voxel: first m picks"""
    return staging.fps(voxel, torch.zeros(voxel.shape[0], dtype=torch.long, device=voxel.device), ratio=m / voxel.shape[0], random_start=False)[:m]


def _loop_stage(cloud_0, cloud_1, centers, final, context, n, m):
    """the parent commit's way: per voxel two torch masks over the whole cloud + staging.stage_pair"""
    fin, ctx = torch.tensor(final, device=DEV), torch.tensor(context, device=DEV)
    out = []
    for k in range(centers.shape[0]):
        c = centers[k]
        v1 = cloud_1[((cloud_1[:, :3] >= c - fin / 2).all(1) & (cloud_1[:, :3] <= c + fin / 2).all(1))]
        v0 = cloud_0[((cloud_0[:, :3] >= c - ctx / 2).all(1) & (cloud_0[:, :3] <= c + ctx / 2).all(1))]
        if v0.shape[0] < m or v1.shape[0] < n:
            continue
        out.append((k,) + tuple(staging.stage_pair(v0, v1, m, n)))
    return out


def test_counts_and_rows_equal_the_reference_lists(fx, scene):
    c0, c1, centers = scene
    for cn, cloud in (("c0", c0), ("c1", c1)):
        for sn, size in (("final", U.FINAL), ("context", U.CONTEXT)):
            off, rows = fx[f"m_{cn}_{sn}_offsets"], fx[f"m_{cn}_{sn}_rows"]
            counts = staging.voxel_counts(cloud, centers, size)
            assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), np.diff(off))
            o, r = staging.voxel_rows(cloud, centers, size)
            assert o.dtype == r.dtype == torch.int64
            assert np.array_equal(o.cpu().numpy(), off) and np.array_equal(r.cpu().numpy(), rows), (cn, sn)
            o2, r2 = staging.voxel_rows(cloud, centers, torch.tensor(size))
            assert torch.equal(o, o2) and torch.equal(r, r2)                      # same input, same bytes
    # planted face / edge / corner rows: in 2, 4 and 8 final boxes
    _, r = staging.voxel_rows(c1, centers, U.FINAL)
    assert torch.bincount(r, minlength=c1.shape[0])[U.PLANT_AT:U.PLANT_AT + 3].tolist() == [2, 4, 8]
    nan = c0.clone()
    nan[0, 1] = float("nan")                                                      # a NaN coordinate is in no box
    assert int(staging.voxel_counts(nan, centers, (100.0, 100.0, 100.0))[0]) == c0.shape[0] - 1


def test_fps_ragged_equals_fps_on_every_cropped_voxel(scene):
    c0, c1, centers = scene
    for cloud, size, m in ((c0, U.CONTEXT, U.N_CONTEXT), (c1, U.FINAL, 64)):     # m = 64: every voxel of the thinned cloud has >= 64 rows
        off, rows = staging.voxel_rows(cloud, centers, size)
        assert int((off[1:] - off[:-1]).min()) >= m
        idx = staging.fps_ragged(cloud, off, rows, m)
        assert idx.shape == (32, m) and idx.dtype == torch.int64
        for k in range(32):
            mem = rows[off[k]:off[k + 1]]
            assert torch.equal(idx[k], mem[_fps_crop(cloud[mem], m)]), k
    # a tie lattice: the 8 x 8 grid of test_fps_ties_batches_and_errors, several voxels of different extents in one cloud
    grid = torch.stack(torch.meshgrid(torch.arange(8.0), torch.arange(8.0), indexing="ij"), -1).reshape(-1, 2)
    parts = [grid[:64], grid[:40] + 100, grid[:17] * 2 - 50, grid[:64].flip(0) + 7]
    cloud = torch.cat(parts).to(DEV).contiguous()
    sizes = [p.shape[0] for p in parts]
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=DEV)
    rows = torch.arange(cloud.shape[0], device=DEV)
    for m in (1, 6, 17):                                                          # m = 1, and m = count of the smallest voxel
        idx = staging.fps_ragged(cloud, off, rows, m)
        for k in range(len(parts)):
            assert torch.equal(idx[k] - off[k], _fps_crop(cloud[off[k]:off[k + 1]], m)), (m, k)
    # rows that are not contiguous, voxels that overlap, m = count
    perm = torch.randperm(cloud.shape[0], generator=torch.Generator().manual_seed(5)).to(DEV)
    lists = [perm[:50].sort().values, perm[20:120].sort().values]
    off2 = torch.tensor([0, 50, 150], dtype=torch.int64, device=DEV)
    idx = staging.fps_ragged(cloud, off2, torch.cat(lists), 50)
    for k, mem in enumerate(lists):
        assert torch.equal(idx[k], mem[_fps_crop(cloud[mem], 50)])
    assert sorted(idx[0].tolist()) == lists[0].tolist()                           # m = count: a permutation of the voxel
    # one voxel above 24576 rows (running distances in the global scratch) next to small ones, in one launch
    big = torch.rand(40000, 6, generator=torch.Generator().manual_seed(9)).to(DEV)
    off3 = torch.tensor([0, 3000, 33000, 40000], dtype=torch.int64, device=DEV)
    idx = staging.fps_ragged(big, off3, torch.arange(40000, device=DEV), 48)
    for k in range(3):
        assert torch.equal(idx[k] - off3[k], _fps_crop(big[off3[k]:off3[k + 1]], 48)), k
    with pytest.raises(RuntimeError, match="fps_ragged"):
        staging.fps_ragged(cloud, off, rows, 18)                                  # the third voxel has 17 rows


def test_stage_scene_equals_the_single_pair_loop_and_the_restatement(fx, scene):
    c0, c1, centers = scene
    st = staging.stage_scene(c0, c1, centers, U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT, ground_height=U.GROUND)
    loop = _loop_stage(c0, c1, centers, U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT)
    assert st.voxel.tolist() == [k for k, *_ in loop] == fx["voxel"].tolist()
    for i, (k, s0, s1, inv) in enumerate(loop):
        assert torch.equal(st.extract_0[i], s0) and torch.equal(st.extract_1[i], s1), k
        assert torch.equal(st.inverse["furthest_distance"][i], inv["furthest_distance"]) and torch.equal(st.inverse["mean"][i], inv["mean"])
        assert torch.equal(st.extra_context[i], (inv["mean"][2] - U.GROUND).unsqueeze(-1))
    assert torch.equal(st.extract_0, torch.stack([s0 for _, s0, _, _ in loop]))
    # rows of the clouds behind the staged points: un-normalising gives them back
    back = st.extract_1[:, :, :3] * st.inverse["furthest_distance"][:, None, None] + st.inverse["mean"][:, None, :]
    assert (back - c1[st.index_1][:, :, :3]).abs().max().item() < 1e-4 and torch.equal(st.extract_1[:, :, 3:], c1[st.index_1][:, :, 3:])
    # the numpy restatement (fp32): tolerances of test_stage_pair_feeds_the_path
    r = U.stage_scene_np(*U.scene(), U.centers_np(), U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT)
    skipped = 0
    for i in range(30):
        same = np.array_equal(st.index_0[i].cpu().numpy(), r["index_0"][i]) and np.array_equal(st.index_1[i].cpu().numpy(), r["index_1"][i])
        if not same:
            _assert_fp64_tie(st, r, i, *U.scene())
            skipped += 1
            continue
        assert np.abs(st.extract_0[i].cpu().numpy() - r["extract_0"][i]).max() < 1e-6
        assert np.abs(st.extract_1[i].cpu().numpy() - r["extract_1"][i]).max() < 1e-6
        assert abs(float(st.inverse["furthest_distance"][i]) - float(r["far"][i])) < 1e-4
    print(f"voxels whose selection differs from the numpy restatement at an fp64 tie: {skipped}")
    assert skipped <= 1
    # and the reference's own co_unit_sphere outputs (fp64) on those rows
    if skipped == 0:
        assert np.abs(st.extract_0[:, :, :3].cpu().double().numpy() - fx["e0_f64"]).max() < 1e-6
        assert np.abs(st.extract_1[:, :, :3].cpu().double().numpy() - fx["e1_f64"]).max() < 1e-6


def _assert_fp64_tie(st, r, i, c0, c1):
    """A selection may differ from the restatement only where, at the first differing pick, both candidates' running distances
    (fp64, to the picks before it) tie within 1e-6 relative."""
    for key, cloud in (("index_0", c0), ("index_1", c1)):
        a, b = st.__dict__[key][i].cpu().numpy(), r[key][i]
        d = np.nonzero(a != b)[0]
        if len(d) == 0:
            continue
        j = d[0]
        prev = cloud[a[:j]].astype(np.float64)
        da, db = (((cloud[p].astype(np.float64) - prev) ** 2).sum(-1).min() for p in (a[j], b[j]))
        print(f"voxel {i} {key}: first differing pick {j}: running distances {da!r} vs {db!r}")
        assert abs(da - db) <= 1e-6 * max(da, db)


def test_validity_and_empty_scenes(fx, scene):
    c0, c1, centers = scene
    st = staging.stage_scene(c0, c1, centers, U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT)
    thin = [k for k in range(32) if k not in st.voxel.tolist()]
    assert len(thin) == 2 and st.extra_context is None
    assert all(int(st.count_1[k]) < U.N_SAMPLES and float(centers[k, 0]) > 3 and float(centers[k, 1]) > 3 for k in thin)
    assert st.voxel.tolist() == sorted(st.voxel.tolist()) and st.voxel.dtype == torch.int64
    assert st.count_0.shape == st.count_1.shape == (32,)
    assert np.array_equal(st.count_0.cpu().numpy(), np.diff(fx["m_c0_context_offsets"]))
    assert np.array_equal(st.count_1.cpu().numpy(), np.diff(fx["m_c1_final_offsets"]))
    assert st.index_0.shape == (30, U.N_CONTEXT) and st.index_1.shape == (30, U.N_SAMPLES)
    none = staging.stage_scene(c0, c1, centers + 1000.0, U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT, ground_height=0.0)
    assert none.extract_0.shape == (0, U.N_CONTEXT, 6) and none.extract_1.shape == (0, U.N_SAMPLES, 6) and none.extra_context.shape == (0, 1)
    assert none.index_0.shape == (0, U.N_CONTEXT) and none.voxel.numel() == 0 and none.inverse["mean"].shape == (0, 3)
    assert int(none.count_0.sum()) == 0 and none.count_0.shape == (32,)
    too_many = staging.stage_scene(c0, c1, centers, U.FINAL, U.CONTEXT, 5000, U.N_CONTEXT)
    assert too_many.voxel.numel() == 0
    off, rows = staging.voxel_rows(c1, centers, U.FINAL)
    with pytest.raises(RuntimeError, match="fps_ragged"):
        staging.fps_ragged(c1, off, rows, U.N_SAMPLES)                            # the thin voxels have fewer rows
    with pytest.raises(RuntimeError, match="GPU"):
        staging.stage_scene(c0.cpu(), c1, centers, U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT)
    with pytest.raises(RuntimeError, match="GPU"):
        staging.voxel_counts(c0[:, :5], centers, U.FINAL)                         # not contiguous


@pytest.fixture(scope="module")
def large():
    """2 M uniform points per cloud in 54 x 54 x 12 m, made on the device: 972 centres of the [3, 3, 4] grid."""
    g = torch.Generator(device=DEV).manual_seed(21)
    lo, ext = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0], device=DEV), torch.tensor([54.0, 54.0, 12.0, 1.0, 1.0, 1.0], device=DEV)
    c0 = (torch.rand(2_000_000, 6, device=DEV, generator=g) * ext + lo).contiguous()
    c1 = (torch.rand(2_000_000, 6, device=DEV, generator=g) * ext + lo).contiguous()
    centers = staging.voxel_centers((0.0, 0.0, 0.0), (54.0, 54.0, 12.0), U.FINAL, device=DEV)
    assert centers.shape == (972, 3)
    return c0, c1, centers


def _mask(cloud, c, size):
    s = torch.tensor(size, device=DEV)
    return (cloud[:, :3] >= c - s / 2).all(1) & (cloud[:, :3] <= c + s / 2).all(1)


def test_large_scene(large):
    c0, c1, centers = large
    for cloud, size in ((c0, U.CONTEXT), (c1, U.FINAL)):
        counts = staging.voxel_counts(cloud, centers, size)
        ref = torch.stack([_mask(cloud, centers[k], size).sum() for k in range(972)])
        assert torch.equal(counts.long(), ref)
        off, rows = staging.voxel_rows(cloud, centers, size)
        for k in torch.randperm(972, generator=torch.Generator().manual_seed(3))[:20].tolist():
            assert torch.equal(rows[off[k]:off[k + 1]], torch.nonzero(_mask(cloud, centers[k], size)).flatten()), k
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = staging.stage_scene(c0, c1, centers, U.FINAL, U.CONTEXT, 1024, 2048)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"stage_scene, 2 x 2 M points, 972 centres, 1024 / 2048 samples: {dt * 1e3:.1f} ms ({st.voxel.numel()} voxels staged; "
          f"target {int(st.count_1.min())}..{int(st.count_1.max())}, context {int(st.count_0.min())}..{int(st.count_0.max())} points per voxel)")
    assert st.voxel.numel() == 972 and st.extract_0.shape == (972, 2048, 6) and st.extract_1.shape == (972, 1024, 6)
    for e in (st.extract_0, st.extract_1):
        assert bool(torch.isfinite(e).all()) and float(e[:, :, :3].abs().max()) <= 1.0


def test_scene_change_equals_the_hand_written_composition(scene):
    c0, c1, centers = scene
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=2, sample_size=U.N_SAMPLES, n_samples_context=U.N_CONTEXT)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    assert cfg["using_extra_context"]
    with pytest.raises(RuntimeError, match="ground_height"):
        fa.scene_change(c0, c1, md, cfg, centers, final_voxel_size=U.FINAL, context_voxel_size=U.CONTEXT)
    with pytest.raises(RuntimeError, match="voxel_size"):
        fa.scene_change(c0, c1, md, cfg, centers, ground_height=U.GROUND)
    kw = dict(ground_height=U.GROUND, multiple=1.0, voxels_per_batch=7)           # multiple = 1: some points of every voxel are marked
    torch.manual_seed(11)
    out, st = fa.scene_change(c0, c1, md, cfg, centers, final_voxel_size=U.FINAL, context_voxel_size=U.CONTEXT, **kw)
    cfg2 = dict(cfg, final_voxel_size=list(U.FINAL), context_voxel_size=list(U.CONTEXT))        # the sizes from the config instead
    torch.manual_seed(11)
    out2, _ = fa.scene_change(c0, c1, md, cfg2, centers, **kw)
    assert torch.equal(out.isnan(), out2.isnan()) and torch.equal(out.nan_to_num(-1.0), out2.nan_to_num(-1.0))

    # by hand
    n, m = U.N_SAMPLES, U.N_CONTEXT
    ok = (staging.voxel_counts(c0, centers, U.CONTEXT) >= m) & (staging.voxel_counts(c1, centers, U.FINAL) >= n) & \
        (staging.voxel_counts(c0, centers, U.FINAL) >= n)
    assert int(ok.sum()) == 30
    sel = centers[ok].contiguous()
    s10 = staging.stage_scene(c0, c1, sel, U.FINAL, U.CONTEXT, n, m, U.GROUND)
    s00 = staging.stage_scene(c0, c0, sel, U.FINAL, U.CONTEXT, n, m, U.GROUND)
    torch.manual_seed(11)
    chunks, sizes = [], []
    for a in range(0, 30, 7):
        ex = s10.extra_context[a:a + 7]
        _, l10, _ = fa.inner_loop((s10.extract_0[a:a + 7], s10.extract_1[a:a + 7], ex), md, cfg)
        _, l00, _ = fa.inner_loop((s00.extract_0[a:a + 7], s00.extract_1[a:a + 7], ex), md, cfg)
        chunks.append(change.log_prob_to_change(l10, l00, 1.0))
        sizes.append(l10.shape[0])
    assert sizes == [7, 7, 7, 7, 2]
    vals = torch.cat(chunks).reshape(-1)
    ref = torch.full((c1.shape[0],), float("nan"), device=DEV)
    ref.scatter_reduce_(0, s10.index_1.reshape(-1), vals, "amax", include_self=False)
    assert torch.equal(out.isnan(), ref.isnan()) and torch.equal(out.nan_to_num(-1.0), ref.nan_to_num(-1.0))
    touched = torch.zeros(c1.shape[0], dtype=torch.bool, device=DEV)
    touched[s10.index_1.reshape(-1)] = True
    assert torch.equal(torch.isfinite(out), touched) and torch.equal(out.isnan(), ~touched)
    assert torch.equal(st.index_1, s10.index_1) and st.voxel.tolist() == torch.nonzero(ok).flatten().tolist() and st.count_0.shape == (32,)
    assert float(out[touched].min()) >= 0.0 and float(out[touched].max()) <= 1.0 and bool((out[touched] > 0).any())


def test_batched_staging_is_at_least_twice_as_fast_as_the_single_pair_loop(large):
    """The floor of DESIGN.md section 11c: 64 valid centres of the large scene, fixture-sized boxes and sample counts; median of 5
    after 2 warm-ups, device synchronisation around the whole staging on both sides."""
    c0, c1, centers = large
    sel = centers[torch.arange(0, 972, 15)[:64]].contiguous()
    assert sel.shape[0] == 64

    def timed(fn):
        ts = []
        for it in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts[2:]), r

    t_loop, loop = timed(lambda: _loop_stage(c0, c1, sel, U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT))
    t_batch, st = timed(lambda: staging.stage_scene(c0, c1, sel, U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT))
    print(f"64 voxels of the 2 x 2 M point scene: single-pair loop {t_loop * 1e3:.1f} ms, stage_scene {t_batch * 1e3:.1f} ms, ratio {t_loop / t_batch:.1f}x")
    assert len(loop) == 64 and st.voxel.numel() == 64
    assert torch.equal(st.extract_0, torch.stack([s0 for _, s0, _, _ in loop])) and torch.equal(st.extract_1, torch.stack([s1 for _, _, s1, _ in loop]))
    assert t_loop >= 2.0 * t_batch
