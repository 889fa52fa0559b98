"""Shared pieces of the scene-staging tests (tests/test_oracle_scene_stage.py, tests/test_gpu_scene_stage.py): the synthetic scene of
the fixture tests/golden/scene_stage_*.npz (regenerated from seeds with tests/golden/synth.py; the fixture stores only what the
reference's own functions returned for it, tests/golden/gen_golden_scene_stage.py) and numpy restatements of box membership
(utils.get_voxel, utils.py:135-142) and of the loader's test-mode item for every voxel of a scene (ams_voxel_loader.py:291-307, 338).
FPS stays `oracle.staging_oracle.fps` (unpinned at reference level: torch_cluster is not available)."""
import os

import numpy as np
import torch

import synth
from oracle import staging_oracle as S

GOLDEN = os.path.dirname(os.path.abspath(synth.__file__))
START, END = (-6.0, -6.0, 0.0), (6.0, 6.0, 8.0)          # a 12 x 12 x 8 m scene
FINAL, CONTEXT = (3.0, 3.0, 4.0), (4.0, 4.0, 5.0)
P0, P1, N_SAMPLES, N_CONTEXT = 24000, 22000, 256, 512
GROUND = 0.25
# planted exactly on faces, edges and corners of the final grid (faces at x, y = -6, -3, 0, 3, 6; z = 0, 4, 8) and of the context boxes
# (centre +- 2 / 2.5): inclusive on both sides, so such a point is in two, four or eight boxes
PLANTED = np.array([[-3.0, 0.7, 1.3], [0.0, 0.0, 2.5], [-3.0, -3.0, 4.0], [3.0, 0.0, 4.0], [-2.5, 0.5, 3.5], [0.5, 0.5, 4.5], [-6.0, -6.0, 0.0],
                    [6.0, 6.0, 8.0], [1.5, 3.0, 4.0], [-2.5, -2.5, 1.0]], dtype=np.float32)
PLANT_AT = 5                                              # first planted row


def _cloud(key, n, thin):
    """n rows [x, y, z, r, g, b] fp32: uniform in the scene; with `thin`, 7 of 8 candidates with x > 3 and y > 3 are dropped."""
    cand = 2 * n
    xyz = np.stack([synth.uniform(f"{key}/{a}", (cand,), lo, hi, seed=7) for a, lo, hi in zip("xyz", START, END)], -1)
    if thin:
        keep = ~((xyz[:, 0] > 3) & (xyz[:, 1] > 3)) | (synth.uniform01(f"{key}/thin", cand, seed=7) < 0.125)
        xyz = xyz[keep]
    pts = np.concatenate([xyz[:n], synth.uniform(f"{key}/rgb", (n, 3), 0.0, 1.0, seed=7)], -1).astype(np.float32)
    assert pts.shape == (n, 6)
    pts[PLANT_AT:PLANT_AT + len(PLANTED), :3] = PLANTED
    return pts


def scene():
    """(cloud_0 [24000, 6], cloud_1 [22000, 6]) float32 numpy; cloud 1 is thinned to 1/8 in the corner column x > 3, y > 3."""
    return _cloud("scene/c0", P0, False), _cloud("scene/c1", P1, True)


def centers_np():
    """utils.get_all_voxel_centers restated: arange(start + size/2, end + size/2, size) per axis, x fastest."""
    ax = [np.arange(np.float32(s) + np.float32(d) / 2, np.float32(e) + np.float32(d) / 2, np.float32(d), dtype=np.float32)
          for s, e, d in zip(START, END, FINAL)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], -1).astype(np.float32)


def members_np(cloud, centers, size):
    """(offsets [K + 1] int64, rows int32): utils.get_voxel's mask per box, fp32 bounds, both inclusive, rows ascending."""
    half = np.asarray(size, dtype=np.float32) / np.float32(2)
    xyz = np.asarray(cloud[:, :3], dtype=np.float32)
    lists = []
    for c in np.asarray(centers, dtype=np.float32):
        lo, hi = (c - half).astype(np.float32), (c + half).astype(np.float32)
        lists.append(np.nonzero(((xyz >= lo) & (xyz <= hi)).all(1))[0].astype(np.int32))
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(l) for l in lists])
    return offsets, (np.concatenate(lists) if lists else np.zeros(0, np.int32))


def fps_first(x, m):
    """first m picks of oracle.staging_oracle.fps on rows x"""
    return S.fps(x, m / x.shape[0])[:m]


def stage_scene_np(cloud_0, cloud_1, centers, final, context, n_samples, n_context, dtype=np.float32):
    """The restated item for every valid voxel: dict with voxel, count_0, count_1, index_0, index_1, extract_0, extract_1, far, mean.
    FPS runs on the fp32 rows (as the loader does); co_unit_sphere in `dtype`."""
    o0, r0 = members_np(cloud_0, centers, context)
    o1, r1 = members_np(cloud_1, centers, final)
    c0, c1 = np.diff(o0), np.diff(o1)
    out = dict(voxel=[], index_0=[], index_1=[], extract_0=[], extract_1=[], far=[], mean=[], count_0=c0.astype(np.int32), count_1=c1.astype(np.int32))
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    for k in range(len(centers)):
        if c0[k] < n_context or c1[k] < n_samples:
            continue
        m0, m1 = r0[o0[k]:o0[k + 1]], r1[o1[k]:o1[k + 1]]
        i0, i1 = m0[fps_first(cloud_0[m0], n_context)], m1[fps_first(cloud_1[m1], n_samples)]
        e0, e1, far, mean = S.co_unit_sphere(torch.from_numpy(cloud_0[i0]).to(tdt), torch.from_numpy(cloud_1[i1]).to(tdt))
        out["voxel"].append(k)
        for key, v in (("index_0", i0), ("index_1", i1), ("extract_0", e0.numpy()), ("extract_1", e1.numpy()), ("far", far.numpy()), ("mean", mean.numpy())):
            out[key].append(v)
    return {k: (np.stack(v) if isinstance(v, list) and v else np.asarray(v)) for k, v in out.items()}


def load_fixture():
    a = dict(np.load(os.path.join(GOLDEN, "scene_stage_members.npz")))
    a.update(np.load(os.path.join(GOLDEN, "scene_stage_sphere.npz")))
    return a
