"""Scene staging with sparse context without a GPU: include/fcflow_sparse_stage.h against abi.SPARSE_STAGE_ENTRIES and the built library,
the refusals that need no device, and the numpy restatement (tests/sparse_stage_util.py) with the inputs of tests/test_gpu_sparse_stage.py
pinned: which voxels of the swapped fixture scene are sparse, and by how much."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import scene_stage_util as U
import sparse_stage_util as SU
from flowcompare_amd import abi, engine, staging
from test_context_counts_host import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcflow_sparse_stage.h")
NAMES = ["fc_stage_fps_ragged_counts_f32", "fc_stage_pairs_counts_f32"]


def test_sparse_stage_table_equals_the_new_header():
    declared = _declared(HEADER)
    assert [n for n, _, _, _ in declared] == list(abi.SPARSE_STAGE_ENTRIES) == NAMES, "names, in the header's order"
    for name, ret, kinds, _ in declared:
        assert abi.SPARSE_STAGE_ENTRIES[name] == (ret, kinds), name
    others = set(abi.ENTRIES) | set(abi.EXTRA_ENTRIES) | set(abi.COUNTS_ENTRIES) | set(abi.DEBUG_ENTRIES)
    assert not set(abi.SPARSE_STAGE_ENTRIES) & others
    text = open(HEADER).read()
    assert '#include "fcflow.h"' in text and "FC_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    pinned = open(os.path.join(ROOT, "include", "fcflow.h")).read()
    assert not any(n in pinned for n in NAMES) and "#define FC_ABI_VERSION 10" in pinned and engine.ABI_VERSION == 10
    # the counts entry is its namesake of fcflow.h with `sample_counts` behind idx
    theirs = {n: (k, names) for n, _, k, names in _declared(os.path.join(ROOT, "include", "fcflow.h"))}
    mine = {n: (k, names) for n, _, k, names in declared}
    kinds, names = mine["fc_stage_fps_ragged_counts_f32"]
    at = names.index("sample_counts")
    assert names[at - 1] == "idx" and kinds[at] == "P"
    assert (kinds[:at] + kinds[at + 1:], names[:at] + names[at + 1:]) == theirs["fc_stage_fps_ragged_f32"]
    assert mine["fc_stage_pairs_counts_f32"][1] == ["cloud_0", "P0", "cloud_1", "P1", "ld", "index_0", "index_1", "counts_0", "n_pairs", "M", "N",
                                                    "out_0", "out_1", "inverse", "stream"]


def test_library_exports_and_binds_the_sparse_stage_entries():
    raw = ctypes.CDLL(engine.LIB_PATH)
    lib = engine.lib()
    for name, (ret, kinds) in abi.SPARSE_STAGE_ENTRIES.items():
        assert hasattr(raw, name), f"{name} not exported"
        assert name in engine.EXTRA_EXPORTS
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [abi.PARAM_KINDS[k] for k in kinds] and fn.restype is abi.RETURN_KINDS[ret], name
        assert fn.errcheck is engine._errcheck, name
    # null pointers are refused with the cause, before a launch (n_voxels / n_pairs = 1: an empty call returns at once)
    with pytest.raises(engine.FcError, match="null pointer"):
        lib.fc_stage_fps_ragged_counts_f32(None, 6, 6, 10, None, None, None, 1, 5, 4, None, 8, None, None)
    with pytest.raises(engine.FcError, match="fc_stage_fps_ragged_counts_f32: bad argument"):
        lib.fc_stage_fps_ragged_counts_f32(None, 6, 6, 10, None, None, None, 1, 5, 4, None, None, None, None)
    with pytest.raises(engine.FcError, match="stage pairs: null pointer"):
        lib.fc_stage_pairs_counts_f32(None, 10, None, 10, 6, None, None, None, 1, 8, 4, None, None, None, None)
    assert lib.fc_stage_pairs_counts_f32(None, 10, None, 10, 6, None, None, None, 0, 8, 4, None, None, None, None) == 0


@pytest.mark.parametrize("bad", [0, SU.M + 1, 2.5, True, torch.tensor(256), "256"])
def test_min_context_is_refused_before_anything_runs(bad):
    """_min_context is the first thing stage_scene and the scene-level functions do with the argument: no tensor is touched before it."""
    with pytest.raises(RuntimeError, match="min_context must"):
        staging._min_context("stage_scene", bad, SU.M)
    assert staging._min_context("stage_scene", None, SU.M) is None and staging._min_context("stage_scene", np.int64(7), SU.M) == 7
    assert staging._min_context("stage_scene", SU.M, SU.M) == SU.M and staging._min_context("stage_scene", 1, SU.M) == 1


@pytest.fixture(scope="module")
def restated():
    c0, c1 = SU.swapped_scene()
    return SU.stage_sparse_np(c0, c1, U.centers_np(), U.FINAL, U.CONTEXT, SU.N, SU.M, 256)


def test_the_swapped_fixture_scene_has_the_sparse_voxels_the_gpu_tests_rely_on(restated):
    r = restated
    c = r["count_0"]
    assert c.shape == (32,) and int((r["count_1"] >= SU.N).sum()) == 32
    assert sorted(c[c < 1000].tolist()) == [400, 403]
    mid = c[(c >= 1000) & (c < SU.M)]
    assert len(mid) == 18 and mid.min() == 1064 and mid.max() == 1273
    assert int((c == SU.M).sum()) == 1
    above = c[c > SU.M]
    assert len(above) == 11 and above.min() == 1302 and above.max() == 1486
    assert int((c >= SU.M).sum()) == 12                                           # what the code stages without min_context
    assert r["voxel"].tolist() == list(range(32)) and int((c >= 512).sum()) == 30
    assert np.array_equal(r["context_counts"], np.minimum(c, SU.M))
    # the unswapped direction: 11 sparse voxels, 1089 .. 1279 points
    o0, _ = U.members_np(SU.swapped_scene()[1], U.centers_np(), U.CONTEXT)
    u = np.diff(o0)
    assert int((u < SU.M).sum()) == 11 and u[u < SU.M].min() == 1089 and u[u < SU.M].max() == 1279


def test_restatement_pads_and_truncates(restated):
    r = restated
    c0, c1 = SU.swapped_scene()
    assert r["extract_0"].shape == (32, SU.M, 6) and r["index_0"].shape == (32, SU.M) and r["extract_1"].shape == (32, SU.N, 6)
    for i in range(32):
        c = int(r["context_counts"][i])
        assert (r["index_0"][i, c:] == -1).all() and (r["extract_0"][i, c:] == 0).all() and (r["index_0"][i, :c] >= 0).all()
        assert len(set(r["index_0"][i, :c].tolist())) == c                        # distinct rows of the context cloud
        if c < SU.M:                                                              # a sparse voxel keeps every member, FPS only orders them
            lo, hi = U.centers_np()[i] - np.float32(U.CONTEXT) / 2, U.centers_np()[i] + np.float32(U.CONTEXT) / 2
            inside = np.nonzero(((c0[:, :3] >= lo) & (c0[:, :3] <= hi)).all(1))[0]
            assert sorted(r["index_0"][i, :c].tolist()) == inside.tolist()
        # joint normalisation of the truncated pair: zero mean over the c + N real rows, the farthest row on the unit sphere
        joint = np.concatenate([r["extract_0"][i, :c, :3], r["extract_1"][i, :, :3]]).astype(np.float64)
        assert np.abs(joint.mean(0)).max() < 1e-6 and abs(np.linalg.norm(joint, axis=1).max() - 1.0) < 1e-6
        assert np.array_equal(r["extract_0"][i, :c, 3:], c0[r["index_0"][i, :c], 3:])
    # a voxel at or above M is U.stage_scene_np's item
    full = U.stage_scene_np(c0, c1, U.centers_np(), U.FINAL, U.CONTEXT, SU.N, SU.M)
    assert len(full["voxel"]) == 12
    for j, k in enumerate(full["voxel"].tolist()):
        assert np.array_equal(full["index_0"][j], r["index_0"][k]) and np.array_equal(full["extract_0"][j], r["extract_0"][k])
        assert np.array_equal(full["extract_1"][j], r["extract_1"][k]) and np.array_equal(full["far"][j], r["far"][k])
