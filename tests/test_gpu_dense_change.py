"""Dense change maps on the GPU: fc_stage_dense_blocks_f32 against the numpy restatement of
tests/dense_change_util.py and the staged sample, fc_change_map_ragged_f32 against fc_change_map_f32 (uniform offsets) and an fp64
restatement (ragged offsets), fa.scene_change(dense=True) against its hand-written composition, and the independence of a point's density
from the batch it sits in.  Scene, fixtures and flow of tests/test_gpu_scene_stage.py."""
import contextlib
import io

import numpy as np
import pytest
import torch

import dense_change_util as D
import flowcompare_amd as fa
import scene_stage_util as U
import synth
from flowcompare_amd import change, engine, staging

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def scene():
    c0, c1 = U.scene()
    return torch.from_numpy(c0).to(DEV), torch.from_numpy(c1).to(DEV), torch.from_numpy(U.centers_np()).to(DEV)


@pytest.fixture(scope="module")
def staged(scene):
    c0, c1, centers = scene
    return staging.stage_scene(c0, c1, centers, U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT, ground_height=U.GROUND)


def _model(**kw):
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=2, sample_size=U.N_SAMPLES, n_samples_context=U.N_CONTEXT, **kw)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    return cfg, md


def _check_blocks(cloud, st, centers_np, dense, block):
    """dense (a DenseStage) against the restatement fed with the GPU's own mean / furthest_distance, and against the staged sample"""
    cl = cloud.cpu().numpy()
    off, rows = U.members_np(cl, centers_np[st.voxel.cpu().numpy()], U.FINAL)
    assert np.array_equal(dense.offsets.cpu().numpy(), off) and np.array_equal(dense.rows.cpu().numpy(), rows)
    blocks, index, block_voxel, block_offsets = D.dense_blocks_np(cl, off, rows, st.inverse["furthest_distance"].cpu().numpy(),
                                                                  st.inverse["mean"].cpu().numpy(), block)
    assert dense.block == block and dense.blocks.shape == blocks.shape and dense.index.dtype == torch.int64 and dense.block_voxel.dtype == torch.int32
    assert np.array_equal(dense.index.cpu().numpy(), index)                       # the member lists, -1 in the pads
    assert np.array_equal(dense.block_voxel.cpu().numpy(), block_voxel) and np.array_equal(dense.block_offsets.cpu().numpy(), block_offsets)
    assert np.array_equal(dense.blocks.cpu().numpy().view(np.uint32), blocks.view(np.uint32))       # bit for bit
    pad = dense.index < 0
    first = dense.blocks[dense.block_offsets[dense.block_voxel.long()], 0]        # the first member of every block's voxel
    assert int(pad.sum()) == int((block * np.diff(block_offsets) - np.diff(off)).sum())
    assert torch.equal(dense.blocks[pad], first[:, None, :].expand_as(dense.blocks)[pad])
    # every FPS pick of every voxel: the dense row has the bits of the staged sample's row
    flat = dense.blocks.reshape(-1, dense.blocks.shape[2])[dense.index.reshape(-1) >= 0]            # CSR order
    for i in range(st.voxel.numel()):
        mem = dense.rows[dense.offsets[i]:dense.offsets[i + 1]]
        pos = torch.searchsorted(mem, st.index_1[i])
        assert torch.equal(mem[pos], st.index_1[i])
        assert torch.equal(flat[dense.offsets[i] + pos], st.extract_1[i]), i
    return off, rows


@pytest.mark.parametrize("block", [256, 96])
def test_blocks_equal_the_restatement_and_the_sample(scene, staged, block):
    c0, c1, centers = scene
    dense = staging.stage_dense(c1, staged, U.FINAL, centers, block)
    _check_blocks(c1, staged, U.centers_np(), dense, block)
    # a row per membership in a STAGED voxel; the planted face / edge / corner points: in 2, 4 and 8 voxels
    times = torch.bincount(dense.rows, minlength=c1.shape[0])
    off_all, rows_all = staging.voxel_rows(c1, centers, U.FINAL)
    valid = torch.zeros(32, dtype=torch.bool, device=DEV)
    valid[staged.voxel] = True
    owner = torch.repeat_interleave(torch.arange(32, device=DEV), off_all[1:] - off_all[:-1])
    assert torch.equal(times, torch.bincount(rows_all[valid[owner]], minlength=c1.shape[0]))
    assert times[U.PLANT_AT:U.PLANT_AT + 3].tolist() == [2, 4, 8]
    # same input, same bytes
    again = staging.stage_dense(c1, staged, U.FINAL, centers, block)
    for key in ("blocks", "index", "block_voxel", "offsets", "rows"):
        assert torch.equal(getattr(dense, key), getattr(again, key)), key
    # a NaN coordinate is in no voxel, so in no block
    nan = c1.clone()
    victim = int(staged.index_1[0, 0])
    nan[victim, 1] = float("nan")
    st_nan = staging.stage_scene(c0, nan, centers, U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT, ground_height=U.GROUND)
    d_nan = staging.stage_dense(nan, st_nan, U.FINAL, centers, block)
    assert int(times[victim]) >= 1 and not bool((d_nan.index == victim).any()) and d_nan.rows.numel() == dense.rows.numel() - int(times[victim])
    assert bool(torch.isfinite(d_nan.blocks).all())


@pytest.mark.parametrize("block", [256, 96])
def test_blocks_of_voxels_with_an_exact_multiple_and_one_more(scene, block):
    c0, c1, _ = scene
    cs_np, (na, nb) = D.special_centres(c1.cpu().numpy(), block)
    cs = torch.from_numpy(cs_np).to(DEV)
    st = staging.stage_scene(c0, c1, cs, U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT, ground_height=U.GROUND)
    assert st.voxel.tolist() == [0, 1, 2]
    dense = staging.stage_dense(c1, st, U.FINAL, cs, block)
    counts = (dense.offsets[1:] - dense.offsets[:-1]).tolist()
    assert counts[:2] == [na, nb] and counts[0] % block == 0 and counts[1] % block == 1     # both cases occur
    _check_blocks(c1, st, cs_np, dense, block)
    per_voxel = torch.bincount(dense.block_voxel.long(), minlength=3).tolist()
    assert per_voxel[:2] == [na // block, nb // block + 1]
    last_a, last_b = int(dense.block_offsets[1]) - 1, int(dense.block_offsets[2]) - 1
    assert int((dense.index[last_a] < 0).sum()) == 0 and int((dense.index[last_b] < 0).sum()) == block - 1   # no pad slot / all but one


def test_voxel_lists_and_refusals(scene, staged):
    c0, c1, centers = scene
    # the C entry with a voxel list: voxels 7, 2, 20 of the full CSR, in that order
    off, rows = staging.voxel_rows(c1, centers, U.FINAL)
    ids = torch.tensor([7, 2, 20], dtype=torch.int32, device=DEV)
    pos = [staged.voxel.tolist().index(k) for k in ids.tolist()]
    inv = torch.cat((staged.inverse["furthest_distance"][pos, None], staged.inverse["mean"][pos]), 1).contiguous()
    cnt = (off[1:] - off[:-1])[ids.long()]
    boff = torch.zeros(4, dtype=torch.int64, device=DEV)
    boff[1:] = torch.cumsum((cnt + 95) // 96, 0)
    blocks, index, block_voxel = engine.stage_dense_blocks(c1, off, rows.to(torch.int32), inv, boff, int(boff[-1]), 96, voxel_ids=ids)
    sub_off = np.concatenate([[0], np.cumsum(cnt.cpu().numpy())])
    sub_rows = np.concatenate([rows[off[k]:off[k + 1]].cpu().numpy() for k in ids.tolist()])
    b_np, i_np, v_np, _ = D.dense_blocks_np(c1.cpu().numpy(), sub_off, sub_rows, inv[:, 0].cpu().numpy(), inv[:, 1:].cpu().numpy(), 96)
    assert np.array_equal(index.cpu().numpy(), i_np) and np.array_equal(block_voxel.cpu().numpy(), v_np)
    assert np.array_equal(blocks.cpu().numpy().view(np.uint32), b_np.view(np.uint32))
    # refusals and the empty stage
    with pytest.raises(RuntimeError, match="block"):
        staging.stage_dense(c1, staged, U.FINAL, centers, 0)
    with pytest.raises(RuntimeError, match="does not belong"):
        staging.stage_dense(c1, staged, U.FINAL, centers[:31].contiguous(), 96)
    with pytest.raises(RuntimeError, match="counts differ"):
        staging.stage_dense(c1, staged, U.CONTEXT, centers, 96)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        staging.stage_dense(c1.cpu(), staged, U.FINAL, centers, 96)
    none = staging.stage_scene(c0, c1, centers + 1000.0, U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT, ground_height=0.0)
    empty = staging.stage_dense(c1, none, U.FINAL, centers + 1000.0, 96)
    assert empty.blocks.shape == (0, 96, 6) and empty.index.shape == (0, 96) and empty.block_voxel.numel() == 0
    assert empty.offsets.tolist() == [0] and empty.rows.numel() == 0 and empty.rows.dtype == torch.int64


# ---------------------------------------------------------------- ragged change map
def _lp(B, n_total, n0, seed):
    g = torch.Generator().manual_seed(seed)
    lp10 = torch.randn(n_total, generator=g) * 4.0 - 8.0
    lp00 = torch.randn(B, n0, generator=g) * 2.0 - 5.0
    return lp10, lp00


@pytest.mark.parametrize("multiple,cutoff", [(1.0, None), (5.4, None), (1.0, -7.0)])
def test_uniform_offsets_equal_the_existing_change_map(multiple, cutoff):
    B, N, N0 = 5, 300, 256
    lp10, lp00 = _lp(B, B * N, N0, 3)
    lp10[[7, 400, 1499]] = float("-inf")
    lp10[[0, 901]] = float("inf")
    lp00[1, 3], lp00[4, 255] = float("inf"), float("-inf")
    a10, a00 = lp10.reshape(B, N).to(DEV), lp00.to(DEV)
    b10, b00 = lp10.to(DEV), lp00.to(DEV)
    offsets = torch.arange(B + 1, device=DEV) * N
    with contextlib.redirect_stdout(io.StringIO()):
        ref = change.log_prob_to_change(a10, a00, multiple, cutoff)
        out = change.log_prob_to_change_ragged(b10, offsets, b00, multiple, cutoff)
    assert out.shape == (B * N,) and torch.equal(out.reshape(B, N), ref)
    assert torch.equal(b10.reshape(B, N), a10) and torch.equal(b00, a00) and not bool(b10.isinf().any()) and not bool(b00.isinf().any())
    assert bool((out > 0).any()) and bool((out == 0).any())


@pytest.mark.parametrize("multiple,cutoff", [(1.0, None), (5.4, None), (1.0, -7.0)])
def test_ragged_offsets_against_fp64(multiple, cutoff):
    counts = [1, 2, 255, 0, 256, 257, 700]
    off_np = np.concatenate([[0], np.cumsum(counts)])
    B, N0 = len(counts), 256
    lp10, lp00 = _lp(B, int(off_np[-1]), N0, 5)
    lp10[0] = 4.0                                                                 # the voxel of one row: unchanged (one changed row alone is 0 / 0)
    lp10[[10, 600, 1400]] = float("-inf")
    lp10[300] = float("inf")
    lp00[2, 9], lp00[6, 0] = float("-inf"), float("inf")
    g10, g00, offsets = lp10.to(DEV), lp00.to(DEV), torch.from_numpy(off_np).to(DEV)
    with contextlib.redirect_stdout(io.StringIO()):
        out = change.log_prob_to_change_ragged(g10, offsets, g00, multiple, cutoff)
    ref, l10, thr = D.change_ragged_f64(lp10, off_np, lp00, multiple, cutoff)
    assert torch.equal(g10.cpu().double(), l10)                                   # clamped in place to the flat tensor's smallest non-inf
    owner = torch.repeat_interleave(torch.arange(B), torch.tensor(counts))
    near = (l10 - thr[owner]).abs() <= 1e-6
    out64 = out.cpu().double()
    assert int(near.sum()) <= 0.01 * near.numel()
    err = (out64 - ref)[~near].abs().max().item()
    print(f"ragged change map, multiple {multiple} cutoff {cutoff}: max |gpu - fp64| {err:.2e}, rows excused at the threshold {int(near.sum())}")
    assert torch.equal((out64 != 0)[~near], (ref != 0)[~near])               # the changed-mask
    assert err <= 1e-6
    # a second run on the clamped input: the same bytes
    with contextlib.redirect_stdout(io.StringIO()):
        again = change.log_prob_to_change_ragged(g10, offsets, g00, multiple, cutoff)
    assert torch.equal(out, again)


def test_ragged_change_map_refusals():
    lp10, lp00 = _lp(2, 10, 8, 1)
    lp10[0] = -50.0                                                               # a voxel of ONE row that counts as changed: 0 / 0, as in the reference
    with pytest.raises(AssertionError):
        change.log_prob_to_change_ragged(lp10.to(DEV), torch.tensor([0, 1, 10], device=DEV), lp00.to(DEV), 1.0)
    with pytest.raises(RuntimeError, match="offsets"):
        change.log_prob_to_change_ragged(lp10.to(DEV), torch.tensor([0, 4, 11], device=DEV), lp00.to(DEV), 1.0)
    with pytest.raises(RuntimeError, match="offsets"):
        change.log_prob_to_change_ragged(lp10.to(DEV), torch.tensor([0, 6, 4, 10], device=DEV), lp00.to(DEV), 1.0)


# ---------------------------------------------------------------- the public entry
def test_dense_scene_change_equals_the_hand_written_composition(scene, monkeypatch):
    c0, c1, centers = scene
    cfg, md = _model()
    kw = dict(ground_height=U.GROUND, multiple=1.0, voxels_per_batch=7, final_voxel_size=U.FINAL, context_voxel_size=U.CONTEXT)
    torch.manual_seed(11)
    out, st = fa.scene_change(c0, c1, md, cfg, centers, dense=True, block=96, **kw)
    torch.manual_seed(11)
    sampled, st_s = fa.scene_change(c0, c1, md, cfg, centers, **kw)

    # by hand
    n, m = U.N_SAMPLES, U.N_CONTEXT
    ok = (staging.voxel_counts(c0, centers, U.CONTEXT) >= m) & (staging.voxel_counts(c1, centers, U.FINAL) >= n) & \
        (staging.voxel_counts(c0, centers, U.FINAL) >= n)
    assert int(ok.sum()) == 30
    sel = centers[ok].contiguous()
    s10 = staging.stage_scene(c0, c1, sel, U.FINAL, U.CONTEXT, n, m, U.GROUND)
    s00 = staging.stage_scene(c0, c0, sel, U.FINAL, U.CONTEXT, n, m, U.GROUND)
    dense = staging.stage_dense(c1, s10, U.FINAL, sel, 96)
    torch.manual_seed(11)
    l10 = fa.dense_log_prob(s10, dense, md, cfg, blocks_per_batch=7)
    l00 = torch.cat([fa.inner_loop((s00.extract_0[a:a + 7], s00.extract_1[a:a + 7], s10.extra_context[a:a + 7]), md, cfg)[1] for a in range(0, 30, 7)])
    assert l10.shape == (dense.rows.numel(),) and l00.shape == (30, n)
    vals = change.log_prob_to_change_ragged(l10, dense.offsets, l00, 1.0)
    ref = torch.full((c1.shape[0],), float("nan"), device=DEV)
    ref.scatter_reduce_(0, dense.rows, vals, "amax", include_self=False)
    assert torch.equal(out.isnan(), ref.isnan()) and torch.equal(out.nan_to_num(-1.0), ref.nan_to_num(-1.0))
    assert torch.equal(st.dense.index, dense.index) and torch.equal(st.dense.rows, dense.rows) and st.dense.block == 96
    assert st.voxel.tolist() == torch.nonzero(ok).flatten().tolist() and st.count_1.shape == (32,)

    # finite exactly on the union of the staged voxels' member rows (numpy lists), values in [0, 1], some marked
    o_np, r_np = U.members_np(c1.cpu().numpy(), U.centers_np()[ok.cpu().numpy()], U.FINAL)
    touched = torch.zeros(c1.shape[0], dtype=torch.bool, device=DEV)
    touched[torch.from_numpy(r_np).long().to(DEV)] = True
    assert torch.equal(torch.isfinite(out), touched) and torch.equal(out.isnan(), ~touched)
    assert int(touched.sum()) > 20000 and int(torch.isfinite(sampled).sum()) <= 30 * n
    assert float(out[touched].min()) >= 0.0 and float(out[touched].max()) <= 1.0 and bool((out[touched] > 0).any())
    corner = (c1[:, 0] > 3) & (c1[:, 1] > 3)                                      # the thinned column: its two voxels fail the validity mask
    assert int(corner.sum()) > 100 and bool(out[corner].isnan().all())

    # dense=False beside it: the sampled composition, as before
    torch.manual_seed(11)
    chunks = []
    for a in range(0, 30, 7):
        ex = s10.extra_context[a:a + 7]
        _, a10, _ = fa.inner_loop((s10.extract_0[a:a + 7], s10.extract_1[a:a + 7], ex), md, cfg)
        _, a00, _ = fa.inner_loop((s00.extract_0[a:a + 7], s00.extract_1[a:a + 7], ex), md, cfg)
        chunks.append(change.log_prob_to_change(a10, a00, 1.0))
    ref_s = torch.full((c1.shape[0],), float("nan"), device=DEV)
    ref_s.scatter_reduce_(0, s10.index_1.reshape(-1), torch.cat(chunks).reshape(-1), "amax", include_self=False)
    assert torch.equal(sampled.isnan(), ref_s.isnan()) and torch.equal(sampled.nan_to_num(-1.0), ref_s.nan_to_num(-1.0))
    assert not hasattr(st_s, "dense")

    # no valid voxel: all NaN, and nothing runs beyond the counts
    def never(*a, **k):
        raise AssertionError("launched for an empty scene")
    for name in ("stage_voxel_select", "stage_fps_ragged", "stage_dense_blocks", "change_map_ragged", "change_map"):
        monkeypatch.setattr(engine, name, never)
    monkeypatch.setattr(type(md["flow"]), "log_prob", never)
    none, st_n = fa.scene_change(c0, c1, md, cfg, centers + 1000.0, dense=True, **kw)
    assert none.shape == (c1.shape[0],) and bool(none.isnan().all())
    assert st_n.dense.blocks.shape == (0, n, 6) and st_n.voxel.numel() == 0 and st_n.count_1.shape == (32,)


def test_dense_log_prob_refusals(scene, staged):
    c0, c1, centers = scene
    cfg, md = _model()
    dense = staging.stage_dense(c1, staged, U.FINAL, centers, 96)
    with pytest.raises(RuntimeError, match="eps"):
        fa.dense_log_prob(staged, dense, md, cfg, eps=[torch.zeros(dense.rows.numel() - 1, 294, device=DEV)])
    with pytest.raises(RuntimeError, match="blocks_per_batch"):
        fa.dense_log_prob(staged, dense, md, cfg, blocks_per_batch=0)
    md["flow"].train()
    with pytest.raises(RuntimeError, match="eval"):
        fa.dense_log_prob(staged, dense, md, cfg)
    md["flow"].eval()


def test_a_points_density_does_not_depend_on_its_batch(scene, staged):
    """Dense log-probs at the FPS-picked rows against flow.log_prob on the sampled batch, augmenter noise zero on both sides; ceiling: the
    project's per-point gate of 2e-3.  Weights: every entry of both state dicts from tests/golden/synth.py's
    synth_state_dict (seed 3), the rule set of the golden generators -- the factory's initial coupling and attention output layers are
    too weak to tell one context from another.  The same comparison with block_voxel rolled by one voxel (every block scored against its
    neighbour's context and extra context) must exceed ten times the observed maximum on most voxels."""
    c0, c1, centers = scene
    cfg, md = _model()
    for part in ("flow", "input_embedder"):
        md[part].load_state_dict(synth.synth_state_dict(md[part].state_dict(), seed=3))
    K1, n = staged.voxel.numel(), U.N_SAMPLES
    dense = staging.stage_dense(c1, staged, U.FINAL, centers, 96)
    width = md["flow"].noise_shapes(1, 1)[0][2]
    lp_s = fa.inner_loop(staged.batch(), md, cfg, eps=[torch.zeros(K1, n, width, device=DEV)])[1]
    zeros = [torch.zeros(dense.rows.numel(), width, device=DEV)]
    lp_d = fa.dense_log_prob(staged, dense, md, cfg, blocks_per_batch=16, eps=zeros)
    assert bool(torch.isfinite(lp_s).all()) and bool(torch.isfinite(lp_d).all())

    def at_picks(lp):
        rows = []
        for i in range(K1):
            mem = dense.rows[dense.offsets[i]:dense.offsets[i + 1]]
            rows.append(lp[dense.offsets[i] + torch.searchsorted(mem, staged.index_1[i])])
        return torch.stack(rows)

    err = (at_picks(lp_d) - lp_s).abs().amax(1)
    worst = float(err.max())
    print(f"dense against sampled log-prob at the FPS picks, zero noise: max {worst:.3e} (mean |log-prob| {float(lp_s.abs().mean()):.2f})")
    assert worst <= 2e-3
    rolled = staging.DenseStage(**dict(dense.__dict__, block_voxel=(dense.block_voxel + 1) % K1))
    err_r = (at_picks(fa.dense_log_prob(staged, rolled, md, cfg, blocks_per_batch=16, eps=zeros)) - lp_s).abs().amax(1)
    seen = int((err_r > 10.0 * worst).sum())
    print(f"with block_voxel rolled by one voxel: per-voxel max between {float(err_r.min()):.3e} and {float(err_r.max()):.3e}; "
          f"above ten times the observed maximum on {seen} of {K1} voxels")
    assert seen > K1 // 2
