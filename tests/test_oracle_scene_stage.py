"""The restatements of tests/scene_stage_util.py (box membership, the loader's item for every voxel of a scene) against golden vectors
produced by the reference's own functions (tests/golden/gen_golden_scene_stage.py), and the host surface of the feature.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import flowcompare_amd as fa
import scene_stage_util as U
from conftest import ROOT
from flowcompare_amd import engine, staging

NEW_EXPORTS = ("fc_stage_voxel_ws_bytes", "fc_stage_voxel_count_f32", "fc_stage_voxel_select_f32", "fc_stage_fps_ragged_f32")


def test_centres_and_member_lists_reproduce_the_reference_exactly():
    fx = U.load_fixture()
    c0, c1 = U.scene()
    centers = U.centers_np()
    assert centers.shape == (32, 3) and np.array_equal(centers, fx["centers"])
    assert torch.equal(staging.voxel_centers(U.START, U.END, U.FINAL), torch.from_numpy(fx["centers"]))
    for cn, cloud in (("c0", c0), ("c1", c1)):
        for sn, size in (("final", U.FINAL), ("context", U.CONTEXT)):
            off, rows = U.members_np(cloud, centers, size)
            assert np.array_equal(off, fx[f"m_{cn}_{sn}_offsets"]) and np.array_equal(rows, fx[f"m_{cn}_{sn}_rows"]), (cn, sn)
    # the planted face / edge / corner points are in 2, 4 and 8 final boxes (bounds inclusive on both sides)
    off, rows = U.members_np(c1, centers, U.FINAL)
    times = np.bincount(rows, minlength=len(c1))[U.PLANT_AT:U.PLANT_AT + 3]
    assert times.tolist() == [2, 4, 8]
    cnt = np.diff(off)
    assert (cnt < U.N_SAMPLES).sum() == 2 and cnt.max() > 600          # the thinned corner column


@pytest.mark.parametrize("dt,tag,tol", [(np.float64, "f64", 1e-12), (np.float32, "f32", 1e-6)])
def test_stage_scene_restatement_reproduces_the_reference(dt, tag, tol):
    fx = U.load_fixture()
    c0, c1 = U.scene()
    r = U.stage_scene_np(c0, c1, U.centers_np(), U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT, dtype=dt)
    assert r["voxel"].tolist() == fx["voxel"].tolist() and len(r["voxel"]) == 30
    assert r["extract_0"].shape == (30, U.N_CONTEXT, 6) and r["extract_1"].shape == (30, U.N_SAMPLES, 6)
    for key, ref in (("extract_0", "e0"), ("extract_1", "e1")):
        err = np.abs(r[key][:, :, :3].astype(np.float64) - fx[f"{ref}_{tag}"]).max()
        print(f"{key} {tag}: max |restatement - reference| {err:.1e}")
        assert err <= tol
    assert np.abs(r["far"] - fx[f"far_{tag}"]).max() <= tol * 100 and np.abs(r["mean"] - fx[f"mean_{tag}"]).max() <= tol * 100
    for k in range(30):                                                 # colour columns pass through; picks start at the voxel's first row
        assert np.array_equal(r["extract_1"][k, :, 3:].astype(np.float32), c1[r["index_1"][k], 3:])
    assert (np.abs(r["extract_0"][:, :, :3]).max() <= 1.0 + 1e-6)


def test_host_surface():
    header = open(os.path.join(ROOT, "include", "fcflow.h")).read()
    for name in NEW_EXPORTS:
        assert name in engine.EXPORTS and re.search(r"\b%s\s*\(" % name, header), name
    assert engine.ABI_VERSION == 10 and "#define FC_ABI_VERSION 10" in header
    for name in ("voxel_centers", "voxel_counts", "voxel_rows", "fps_ragged", "stage_scene"):
        assert callable(getattr(staging, name)), name
    assert callable(fa.scene_change) and "scene_change" in fa.__all__


def test_cpu_tensors_are_refused():
    c0, c1 = (torch.from_numpy(c) for c in U.scene())
    centers = torch.from_numpy(U.centers_np())
    with pytest.raises(RuntimeError, match="GPU"):
        staging.stage_scene(c0, c1, centers, U.FINAL, U.CONTEXT, U.N_SAMPLES, U.N_CONTEXT)
    with pytest.raises(RuntimeError, match="GPU"):
        staging.voxel_counts(c0, centers, U.FINAL)
    with pytest.raises(RuntimeError, match="GPU"):
        staging.voxel_rows(c0.double(), centers, U.FINAL)
    with pytest.raises(RuntimeError, match="GPU"):
        staging.fps_ragged(c0, torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 1)
