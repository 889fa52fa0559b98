"""Host surface of the dense change maps and the numpy restatement of the block layout on the synthetic scene.
No GPU."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import dense_change_util as D
import flowcompare_amd as fa
import scene_stage_util as U
from conftest import ROOT
from flowcompare_amd import change, engine, staging

NEW_EXPORTS = ("fc_stage_dense_blocks_f32", "fc_change_map_ragged_f32")


def test_the_library_exports_both_entries():
    header = open(os.path.join(ROOT, "include", "fcflow.h")).read()
    assert os.path.exists(engine.LIB_PATH), "libfcflow.so is not built"
    L = ctypes.CDLL(engine.LIB_PATH)
    for name in NEW_EXPORTS:
        assert hasattr(L, name), name
        assert name in engine.EXPORTS and re.search(r"\b%s\s*\(" % name, header), name
    # additions: declared after everything that was there, no version step
    assert header.index("fc_stage_dense_blocks_f32(") > header.index("fc_train_adam_f32(") and engine.ABI_VERSION == 10


def test_public_surface():
    sig = inspect.signature(fa.scene_change)
    assert sig.parameters["dense"].default is False and sig.parameters["block"].default is None
    assert callable(fa.dense_log_prob) and "dense_log_prob" in fa.__all__
    assert list(inspect.signature(fa.dense_log_prob).parameters) == ["st", "dense", "models_dict", "config", "blocks_per_batch", "eps"]
    assert callable(staging.stage_dense) and callable(change.log_prob_to_change_ragged)


def test_cpu_tensors_are_refused():
    c0, c1 = (torch.from_numpy(c) for c in U.scene())
    centers = torch.from_numpy(U.centers_np())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        staging.stage_dense(c1, None, U.FINAL, centers, 256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        change.log_prob_to_change_ragged(torch.zeros(6), torch.tensor([0, 2, 6]), torch.zeros(2, 4), 1.0)
    st = types.SimpleNamespace(extract_0=torch.zeros(1, 8, 6))
    dense = types.SimpleNamespace(blocks=torch.zeros(1, 4, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.dense_log_prob(st, dense, {}, {})


def test_block_restatement_on_the_synthetic_scene():
    _, c1 = U.scene()
    centers = U.centers_np()
    off, rows = U.members_np(c1, centers, U.FINAL)
    far, mean = np.full(32, 2.5, np.float32), centers.astype(np.float32)
    blocks, index, block_voxel, block_offsets = D.dense_blocks_np(c1, off, rows, far, mean, 96)
    counts = np.diff(off)
    assert blocks.shape == (int(((counts + 95) // 96).sum()), 96, 6) and block_offsets[-1] == blocks.shape[0]
    assert np.array_equal(index[index >= 0], rows)                                # masking the slots leaves CSR order
    assert np.array_equal(np.bincount(block_voxel, minlength=32), (counts + 95) // 96)
    pad = index < 0
    first = blocks[block_offsets[block_voxel], 0]                                 # every block's voxel's first member
    assert pad.sum() == (96 * ((counts + 95) // 96) - counts).sum()
    assert np.array_equal(blocks[pad], np.broadcast_to(first[:, None, :], blocks.shape)[pad])
    assert np.array_equal(blocks[~pad][:, 3:], c1[rows][:, 3:])
    for blk in (96, 256):
        cs, (na, nb) = D.special_centres(c1, blk)
        o, _ = U.members_np(c1, cs, U.FINAL)
        assert np.diff(o)[:2].tolist() == [na, nb] and na % blk == 0 and nb % blk == 1 and min(na, nb) >= U.N_SAMPLES
