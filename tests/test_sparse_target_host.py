"""Change maps of voxels with few target points without a GPU: include/fcflow_sparse_target.h against
abi.SPARSE_TARGET_ENTRIES and the built library, the argument rules of `min_target` / `target_counts` (refused before any tensor is touched),
and the numpy restatement (tests/sparse_target_util.py) with the inputs of tests/test_gpu_sparse_target.py pinned: which final boxes of the
fixture scene are thin, and how many voxels each rule stages."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import flowcompare_amd as fa
import scene_stage_util as U
import sparse_stage_util as SU
import sparse_target_util as TU
from flowcompare_amd import abi, engine, model_initialization, staging
from test_context_counts_host import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcflow_sparse_target.h")
NAMES = ["fc_stage_pairs_counts2_f32", "fc_change_map_counts_f32", "fc_change_map_ragged_counts_f32"]


# ---------------------------------------------------------------- ABI table and exports
def test_sparse_target_table_equals_the_new_header():
    declared = _declared(HEADER)
    assert [n for n, _, _, _ in declared] == list(abi.SPARSE_TARGET_ENTRIES) == NAMES, "names, in the header's order"
    for name, ret, kinds, _ in declared:
        assert abi.SPARSE_TARGET_ENTRIES[name] == (ret, kinds), name
    others = set(abi.ENTRIES) | set(abi.EXTRA_ENTRIES) | set(abi.COUNTS_ENTRIES) | set(abi.SPARSE_STAGE_ENTRIES) | set(abi.EMBED_COUNTS_ENTRIES) | \
        set(abi.DEBUG_ENTRIES)
    assert not set(abi.SPARSE_TARGET_ENTRIES) & others
    text = open(HEADER).read()
    assert '#include "fcflow.h"' in text and "FC_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    pinned = open(os.path.join(ROOT, "include", "fcflow.h")).read()
    assert not any(n in pinned for n in NAMES) and "#define FC_ABI_VERSION 10" in pinned and engine.ABI_VERSION == 10
    # every entry is its namesake with the count arrays added: counts_1 behind counts_0 / lp10's N, counts_0 behind lp00's N0
    mine = {n: (k, names) for n, _, k, names in declared}
    theirs = {n: (k, names) for n, _, k, names in _declared(os.path.join(ROOT, "include", "fcflow.h")) +
              _declared(os.path.join(ROOT, "include", "fcflow_sparse_stage.h"))}

    def without(entry, *added):
        kinds, names = mine[entry]
        keep = [i for i, n in enumerate(names) if n not in added]
        assert all(kinds[names.index(a)] == "P" for a in added), entry
        return "".join(kinds[i] for i in keep), [names[i] for i in keep]

    assert without("fc_stage_pairs_counts2_f32", "counts_1") == theirs["fc_stage_pairs_counts_f32"]
    assert mine["fc_stage_pairs_counts2_f32"][1][7:9] == ["counts_0", "counts_1"]
    assert without("fc_change_map_counts_f32", "counts_1", "counts_0") == theirs["fc_change_map_f32"]
    assert mine["fc_change_map_counts_f32"][1][:6] == ["lp10", "N", "counts_1", "lp00", "N0", "counts_0"]
    assert without("fc_change_map_ragged_counts_f32", "counts_0") == theirs["fc_change_map_ragged_f32"]
    assert mine["fc_change_map_ragged_counts_f32"][1][:5] == ["lp10", "offsets", "lp00", "N0", "counts_0"]


def test_library_exports_and_binds_the_sparse_target_entries():
    raw = ctypes.CDLL(engine.LIB_PATH)
    lib = engine.lib()
    for name, (ret, kinds) in abi.SPARSE_TARGET_ENTRIES.items():
        assert hasattr(raw, name), f"{name} not exported"
        assert name in engine.EXTRA_EXPORTS
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [abi.PARAM_KINDS[k] for k in kinds] and fn.restype is abi.RETURN_KINDS[ret], name
        assert fn.errcheck is engine._errcheck, name
    # null pointers are refused with the cause, before a launch or an allocation
    with pytest.raises(engine.FcError, match="stage pairs: null pointer"):
        lib.fc_stage_pairs_counts2_f32(None, 10, None, 10, 6, None, None, None, None, 1, 8, 4, None, None, None, None)
    with pytest.raises(engine.FcError, match="fc_stage_pairs_counts2_f32: bad argument"):
        lib.fc_stage_pairs_counts2_f32(None, 10, None, 10, 6, None, None, None, None, -1, 8, 4, None, None, None, None)
    assert lib.fc_stage_pairs_counts2_f32(None, 10, None, 10, 6, None, None, None, None, 0, 8, 4, None, None, None, None) == 0
    bad = ctypes.c_int32(0)
    with pytest.raises(engine.FcError, match="fc_change_map_counts_f32: null pointer"):
        lib.fc_change_map_counts_f32(None, 4, None, None, 4, None, None, 1, 1.0, 0.0, 0, ctypes.byref(bad), None)
    with pytest.raises(engine.FcError, match="fc_change_map_ragged_counts_f32: null pointer"):
        lib.fc_change_map_ragged_counts_f32(None, None, None, 4, None, None, 1, 1.0, 0.0, 0, ctypes.byref(bad), None)
    assert "min_target" in fa.scene_change.__code__.co_varnames and "target_counts" in fa.inner_loop.__code__.co_varnames
    assert callable(fa.pad_target_batch) and callable(engine.stage_pairs_counts2) and callable(engine.change_map_counts)


# ---------------------------------------------------------------- argument rules
@pytest.mark.parametrize("bad", [0, TU.N + 1, 2.5, True, torch.tensor(64), "64"])
def test_min_target_is_refused_before_anything_runs(bad):
    """_min_target is the first thing stage_scene does with the argument: no tensor is touched before it."""
    with pytest.raises(RuntimeError, match="min_target must"):
        staging._min_target("stage_scene", bad, TU.N)
    assert staging._min_target("stage_scene", None, TU.N) is None and staging._min_target("stage_scene", np.int64(7), TU.N) == 7
    assert staging._min_target("stage_scene", TU.N, TU.N) == TU.N and staging._min_target("stage_scene", 1, TU.N) == 1


def _md(training=False, sharded=False):
    md = {"flow": types.SimpleNamespace(training=training), "input_embedder": types.SimpleNamespace(training=False)}
    if sharded:
        md["sharded"] = True
    return md


def test_scene_level_min_target_starts_at_two_and_says_why():
    cfg = {"sample_size": TU.N, "n_samples_context": TU.M}
    for what in ("scene_change", "scene_context_attribution"):
        with pytest.raises(RuntimeError, match=rf"{what}: min_target must lie in \[2, n_samples = {TU.N}\], got 1 .*unbiased std needs two"):
            model_initialization._scene_min_target(what, 1, _md(), cfg)
        for bad in (0, TU.N + 1, 2.5, True, torch.tensor(64)):
            with pytest.raises(RuntimeError, match=f"{what}: min_target must"):
                model_initialization._scene_min_target(what, bad, _md(), cfg)
        assert model_initialization._scene_min_target(what, None, _md(training=True), cfg) is None
        assert model_initialization._scene_min_target(what, 2, _md(), cfg) == 2 and model_initialization._scene_min_target(what, TU.N, _md(), cfg) == TU.N
        with pytest.raises(RuntimeError, match=f"{what}: min_target is eval-mode only"):
            model_initialization._scene_min_target(what, 64, _md(training=True), cfg)
        with pytest.raises(RuntimeError, match=f"{what}: min_target is not supported with a sharded models_dict"):
            model_initialization._scene_min_target(what, 64, _md(sharded=True), cfg)
    # the scene-level functions check it before they look at a cloud: None stands for every tensor here
    cfg.update(final_voxel_size=U.FINAL, context_voxel_size=U.CONTEXT)
    with pytest.raises(RuntimeError, match="scene_change: min_target must"):
        fa.scene_change(None, None, _md(), cfg, None, min_target=1)
    with pytest.raises(RuntimeError, match="scene_context_attribution: min_target must"):
        fa.scene_context_attribution(None, None, _md(), cfg, None, min_target=TU.N + 1)


def test_target_counts_is_refused_before_anything_runs():
    cfg = {"input_dim": 6, "global": False}
    cpu = torch.zeros(2, 8, 6)
    with pytest.raises(RuntimeError, match="inner_loop: target_counts is eval-mode only"):
        fa.inner_loop((None, None, None), _md(training=True), cfg, target_counts=torch.tensor([1, 2]))
    with pytest.raises(RuntimeError, match="inner_loop: target_counts is not supported with a sharded models_dict"):
        fa.inner_loop((None, None, None), _md(sharded=True), cfg, target_counts=torch.tensor([1, 2]))
    with pytest.raises(RuntimeError, match="tensors must live on a HIP device"):
        fa.inner_loop((cpu, cpu, None), _md(), cfg, target_counts=torch.tensor([1, 2]))
    # the tensor's own rules (engine._context_counts_range with the target's name): type, dtype and device come before any read-back
    for bad, why in ((3, "must be None or an integer tensor"), ([1, 2], "must be None or an integer tensor"),
                     (torch.tensor([1.0, 2.0]), "must be an integer tensor"), (torch.tensor([True, False]), "must be an integer tensor"),
                     (torch.tensor([1, 2]), "must live on a HIP device")):
        with pytest.raises(RuntimeError, match=f"target_counts {why}"):
            engine._context_counts_range(bad, 2, 8, "cpu", "target_counts", side="target")
    with pytest.raises(RuntimeError, match="pad_target_batch: no clouds given"):
        fa.pad_target_batch([])
    with pytest.raises(RuntimeError, match="pad_target_batch: cloud 0 must be a tensor on a HIP device"):
        fa.pad_target_batch([cpu[0]])


# ---------------------------------------------------------------- the fixture scene's thin final boxes, and the numpy restatement
@pytest.fixture(scope="module")
def boxes():
    c0, c1 = U.scene()
    cen = U.centers_np()
    count = lambda cloud, size: np.diff(U.members_np(cloud, cen, size)[0])
    return dict(c0_ctx=count(c0, U.CONTEXT), c1_ctx=count(c1, U.CONTEXT), c0_fin=count(c0, U.FINAL), c1_fin=count(c1, U.FINAL))


def test_the_fixture_scene_has_the_thin_final_boxes_the_gpu_tests_rely_on(boxes):
    b = boxes
    N, M = TU.N, TU.M
    assert (N, M) == (720, 1024) and b["c1_fin"].shape == (32,)
    assert int(b["c0_ctx"].min()) == 1089                                         # context never decides
    thin = np.nonzero(b["c1_fin"] < 200)[0]
    assert thin.tolist() == [15, 31] and b["c1_fin"][thin].tolist() == [103, 89]   # the corner column, both layers
    rest = np.delete(b["c1_fin"], thin)
    assert rest.min() == 678 and rest.max() == 767
    assert b["c0_fin"].min() == 711 and b["c0_fin"].max() == 817
    assert int((b["c1_fin"] < N).sum()) == 13 and int((b["c0_fin"] < N).sum()) == 3
    ctx = b["c0_ctx"] >= M
    # the parent's rules: stage_scene looks at the context box and the (1 | 0) final box, scene_change also at the (0 | 0) final box
    assert int((ctx & (b["c1_fin"] >= N)).sum()) == 19 and int((ctx & (b["c1_fin"] >= N) & (b["c0_fin"] >= N)).sum()) == 17
    for mt, valid in ((64, 32), (96, 31), (104, 30), (N, 19)):
        assert int((ctx & (b["c1_fin"] >= mt)).sum()) == valid, mt
        if mt < N:
            assert int((ctx & (b["c1_fin"] >= mt) & (b["c0_fin"] >= mt)).sum()) == valid, mt
    assert int(np.nonzero(~(b["c1_fin"] >= 96))[0][0]) == 31                       # the 89-point box drops at 96


@pytest.fixture(scope="module")
def restated():
    c0, c1 = U.scene()
    return TU.stage_target_np(c0, c1, U.centers_np(), U.FINAL, U.CONTEXT, TU.N, TU.M, TU.MIN_TARGET)


def test_restatement_pads_and_truncates(restated, boxes):
    r = restated
    c0, c1 = U.scene()
    N, M = TU.N, TU.M
    assert r["voxel"].tolist() == list(range(32)) and np.array_equal(r["target_counts"], np.minimum(boxes["c1_fin"], N))
    assert (r["context_counts"] == M).all() and (r["index_0"] >= 0).all()
    assert r["extract_1"].shape == (32, N, 6) and r["index_1"].shape == (32, N) and r["extract_0"].shape == (32, M, 6)
    assert int((r["target_counts"] < N).sum()) == 13 and sorted(r["target_counts"].tolist())[:3] == [89, 103, 678]
    for i in range(32):
        n = int(r["target_counts"][i])
        assert (r["index_1"][i, n:] == -1).all() and (r["extract_1"][i, n:] == 0).all() and (r["index_1"][i, :n] >= 0).all()
        assert len(set(r["index_1"][i, :n].tolist())) == n
        if n < N:                                                                 # a thin box keeps every member, FPS only orders them
            lo, hi = U.centers_np()[i] - np.float32(U.FINAL) / 2, U.centers_np()[i] + np.float32(U.FINAL) / 2
            inside = np.nonzero(((c1[:, :3] >= lo) & (c1[:, :3] <= hi)).all(1))[0]
            assert sorted(r["index_1"][i, :n].tolist()) == inside.tolist()
        joint = np.concatenate([r["extract_0"][i, :, :3], r["extract_1"][i, :n, :3]]).astype(np.float64)
        assert np.abs(joint.mean(0)).max() < 1e-6 and abs(np.linalg.norm(joint, axis=1).max() - 1.0) < 1e-6
        assert np.array_equal(r["extract_1"][i, :n, 3:], c1[r["index_1"][i, :n], 3:])
    # a voxel with a full final box is U.stage_scene_np's item
    full = U.stage_scene_np(c0, c1, U.centers_np(), U.FINAL, U.CONTEXT, N, M)
    assert len(full["voxel"]) == 19
    for j, k in enumerate(full["voxel"].tolist()):
        assert np.array_equal(full["index_1"][j], r["index_1"][k]) and np.array_equal(full["extract_1"][j], r["extract_1"][k])
        assert np.array_equal(full["extract_0"][j], r["extract_0"][k]) and np.array_equal(full["far"][j], r["far"][k])
    # min_target = 96 drops the 89-point box and nothing else
    r96 = TU.stage_target_np(c0, c1, U.centers_np()[24:], U.FINAL, U.CONTEXT, N, M, 96)
    assert r96["voxel"].tolist() == list(range(7)) and np.array_equal(r96["index_1"], r["index_1"][24:31])


def test_combined_with_min_context_on_the_swapped_scene(boxes):
    """Cloud 0 as the target (711 .. 817 points per final box), the thinned cloud as context: N = 750, M = 1280, min_context = 256, min_target = 700."""
    b = boxes
    N, M = 750, 1280
    ctx, fin = b["c1_ctx"], b["c0_fin"]
    assert int(((ctx >= M) & (fin >= N)).sum()) == 5 and int(((ctx >= 256) & (fin >= N)).sum()) == 15
    assert int(((ctx >= M) & (fin >= 700)).sum()) == 12 and int(((ctx >= 256) & (fin >= 700)).sum()) == 32
    c0, c1 = SU.swapped_scene()
    cen = U.centers_np()[12:18]                                                   # six voxels are enough for the restatement's own rules
    r = TU.stage_target_np(c0, c1, cen, U.FINAL, U.CONTEXT, N, M, 700, min_context=256)
    assert r["voxel"].tolist() == list(range(6))
    assert np.array_equal(r["context_counts"], np.minimum(ctx[12:18], M)) and np.array_equal(r["target_counts"], np.minimum(fin[12:18], N))
    assert (r["context_counts"] < M).any() and (r["target_counts"] < N).any()
    for i in range(6):
        c, n = int(r["context_counts"][i]), int(r["target_counts"][i])
        assert (r["index_0"][i, c:] == -1).all() and (r["extract_0"][i, c:] == 0).all() and (r["index_1"][i, n:] == -1).all()
        assert (r["extract_1"][i, n:] == 0).all()
        joint = np.concatenate([r["extract_0"][i, :c, :3], r["extract_1"][i, :n, :3]]).astype(np.float64)
        assert np.abs(joint.mean(0)).max() < 1e-6 and abs(np.linalg.norm(joint, axis=1).max() - 1.0) < 1e-6
    # with min_context alone the same voxels are SU.stage_sparse_np's items where the final box is full
    s = SU.stage_sparse_np(c0, c1, cen, U.FINAL, U.CONTEXT, N, M, 256)
    for j, k in enumerate(s["voxel"].tolist()):
        assert np.array_equal(s["extract_0"][j], r["extract_0"][k]) and np.array_equal(s["extract_1"][j], r["extract_1"][k])
