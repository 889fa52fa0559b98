"""Shared pieces of the sparse-staging tests (tests/test_sparse_stage_host.py, tests/test_gpu_sparse_stage.py): the fixture scene of
tests/scene_stage_util.py with the roles SWAPPED -- context = cloud 1 (thinned to 1/8 in the corner column x > 3, y > 3), target = cloud 0 --
so that context boxes hold anything from 400 to 1486 points, and the numpy restatement of scene staging with `min_context`."""
import numpy as np
import torch

import scene_stage_util as U
from oracle import staging_oracle as S

M, N = 1280, 64                                           # n_samples_context, n_samples of every test here


def swapped_scene():
    """(cloud_0 = context cloud [22000, 6], cloud_1 = target cloud [24000, 6]) float32 numpy: U.scene() the other way round."""
    c0, c1 = U.scene()
    return c1, c0


def stage_sparse_np(cloud_0, cloud_1, centers, final, context, n_samples, n_context, min_context):
    """U.stage_scene_np's per-voxel item with min(count, n_context) context samples: a voxel is valid when count_0 >= min_context and
    count_1 >= n_samples; extract_0 / index_0 are padded to n_context rows with 0.0 / -1.  fp32 throughout, FPS = oracle.staging_oracle.fps,
    normalisation = oracle.staging_oracle.co_unit_sphere on the truncated pair.  Adds context_counts to the dict."""
    o0, r0 = U.members_np(cloud_0, centers, context)
    o1, r1 = U.members_np(cloud_1, centers, final)
    c0, c1 = np.diff(o0), np.diff(o1)
    out = dict(voxel=[], index_0=[], index_1=[], extract_0=[], extract_1=[], far=[], mean=[], context_counts=[])
    for k in range(len(centers)):
        if c0[k] < min_context or c1[k] < n_samples:
            continue
        m0, m1 = r0[o0[k]:o0[k + 1]], r1[o1[k]:o1[k + 1]]
        c = min(int(c0[k]), n_context)
        i0, i1 = m0[U.fps_first(cloud_0[m0], c)], m1[U.fps_first(cloud_1[m1], n_samples)]
        e0, e1, far, mean = S.co_unit_sphere(torch.from_numpy(cloud_0[i0]), torch.from_numpy(cloud_1[i1]))
        pad_e = np.zeros((n_context, cloud_0.shape[1]), np.float32)
        pad_e[:c] = e0.numpy()
        pad_i = np.full(n_context, -1, np.int64)
        pad_i[:c] = i0
        for key, v in (("voxel", k), ("index_0", pad_i), ("index_1", i1.astype(np.int64)), ("extract_0", pad_e), ("extract_1", e1.numpy()),
                       ("far", far.numpy()), ("mean", mean.numpy()), ("context_counts", c)):
            out[key].append(v)
    out = {k: np.asarray(v) for k, v in out.items()}
    out["count_0"], out["count_1"] = c0.astype(np.int32), c1.astype(np.int32)
    return out
