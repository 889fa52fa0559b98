"""Shared pieces of the sparse-target tests (tests/test_sparse_target_host.py, tests/test_gpu_sparse_target.py): the fixture scene of
tests/scene_stage_util.py in its own direction -- context = cloud 0, target = cloud 1, whose corner column x > 3, y > 3 is thinned to 1/8, so
that two of its 32 final boxes hold 89 and 103 points and the other 30 hold 678 .. 767 -- and the numpy restatement of scene staging with
`min_target` (and, optionally, `min_context`): tests/sparse_stage_util.stage_sparse_np's idea on both sides."""
import numpy as np
import torch

import scene_stage_util as U
from oracle import staging_oracle as S

M, N = 1024, 720                                          # n_samples_context, n_samples: every context box of cloud 0 holds >= 1089 points
MIN_TARGET = 64


def assert_fp64_tie(a, b, cloud, what):
    """The rule of the scene-staging tests for a selection that differs from the numpy restatement: allowed only where, at the first differing
    pick, both candidates' running distances (fp64, to the picks before it) tie within 1e-6 relative."""
    d = np.nonzero(a != b)[0]
    if len(d) == 0:
        return
    j = d[0]
    prev = cloud[a[:j]].astype(np.float64)
    da, db = (((cloud[p].astype(np.float64) - prev) ** 2).sum(-1).min() for p in (a[j], b[j]))
    print(f"{what}: first differing pick {j}: running distances {da!r} vs {db!r}")
    assert abs(da - db) <= 1e-6 * max(da, db)


def stage_target_np(cloud_0, cloud_1, centers, final, context, n_samples, n_context, min_target, min_context=None):
    """U.stage_scene_np's per-voxel item with min(count_1, n_samples) target samples and, with min_context, min(count_0, n_context) context
    samples: a voxel is valid when count_0 >= (min_context or n_context) and count_1 >= min_target; extract / index of either side are padded to
    their sample count with 0.0 / -1.  fp32 throughout, FPS = oracle.staging_oracle.fps, normalisation = oracle.staging_oracle.co_unit_sphere on
    the truncated pair.  Adds context_counts and target_counts to the dict."""
    o0, r0 = U.members_np(cloud_0, centers, context)
    o1, r1 = U.members_np(cloud_1, centers, final)
    c0, c1 = np.diff(o0), np.diff(o1)
    out = dict(voxel=[], index_0=[], index_1=[], extract_0=[], extract_1=[], far=[], mean=[], context_counts=[], target_counts=[])
    C = cloud_0.shape[1]

    def padded(e, i, rows):
        pe, pi = np.zeros((rows, C), np.float32), np.full(rows, -1, np.int64)
        pe[:len(i)], pi[:len(i)] = e, i
        return pe, pi

    for k in range(len(centers)):
        if c0[k] < (n_context if min_context is None else min_context) or c1[k] < min_target:
            continue
        m0, m1 = r0[o0[k]:o0[k + 1]], r1[o1[k]:o1[k + 1]]
        c, n = min(int(c0[k]), n_context), min(int(c1[k]), n_samples)
        i0, i1 = m0[U.fps_first(cloud_0[m0], c)], m1[U.fps_first(cloud_1[m1], n)]
        e0, e1, far, mean = S.co_unit_sphere(torch.from_numpy(cloud_0[i0]), torch.from_numpy(cloud_1[i1]))
        (pe0, pi0), (pe1, pi1) = padded(e0.numpy(), i0, n_context), padded(e1.numpy(), i1, n_samples)
        for key, v in (("voxel", k), ("index_0", pi0), ("index_1", pi1), ("extract_0", pe0), ("extract_1", pe1), ("far", far.numpy()),
                       ("mean", mean.numpy()), ("context_counts", c), ("target_counts", n)):
            out[key].append(v)
    out = {k: np.asarray(v) for k, v in out.items()}
    out["count_0"], out["count_1"] = c0.astype(np.int32), c1.astype(np.int32)
    return out
