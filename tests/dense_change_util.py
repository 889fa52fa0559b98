"""Shared pieces of the dense change-map tests (tests/test_dense_change_host.py, tests/test_gpu_dense_change.py): the numpy restatement of
the block layout of fc_stage_dense_blocks_f32, centres of the synthetic scene of tests/scene_stage_util.py whose
boxes hold an exact multiple of a block size (and a multiple plus one), and the fp64 restatement of the ragged change map
(test_flow.py:241-275 per voxel)."""
import numpy as np
import torch

import scene_stage_util as U


def dense_blocks_np(cloud, offsets, rows, far, mean, block):
    """(blocks [n_blocks, block, C] fp32, index [n_blocks, block] int64, block_voxel [n_blocks] int32, block_offsets [K + 1] int64).
    Voxel i owns ceil(count / block) blocks of its member rows in list order; xyz = (x - mean) / far in fp32 (one rounding per
    operation); a slot beyond the count repeats the voxel's first member with index -1."""
    cloud = np.asarray(cloud, dtype=np.float32)
    far, mean = np.asarray(far, dtype=np.float32), np.asarray(mean, dtype=np.float32)
    counts = np.diff(offsets)
    block_offsets = np.zeros(len(counts) + 1, dtype=np.int64)
    block_offsets[1:] = np.cumsum((counts + block - 1) // block)
    n_blocks, C = int(block_offsets[-1]), cloud.shape[1]
    blocks = np.zeros((n_blocks, block, C), dtype=np.float32)
    index = np.full((n_blocks, block), -1, dtype=np.int64)
    block_voxel = np.zeros(n_blocks, dtype=np.int32)
    for i, n in enumerate(counts):
        mem = np.asarray(rows[offsets[i]:offsets[i + 1]], dtype=np.int64)
        for b in range(int(block_offsets[i + 1] - block_offsets[i])):
            part = mem[b * block:(b + 1) * block]
            src = np.concatenate([part, np.full(block - len(part), mem[0], dtype=np.int64)])
            pts = cloud[src].copy()
            pts[:, :3] = ((pts[:, :3] - mean[i][None, :]).astype(np.float32) / far[i]).astype(np.float32)
            g = int(block_offsets[i]) + b
            blocks[g], block_voxel[g] = pts, i
            index[g, :len(part)] = part
    return blocks, index, block_voxel, block_offsets


def centre_with_count(cloud, start, size, block, residue, at_least):
    """`start` [3], a centre whose box touches the scene's x = -6 m side, moved outwards in fp32 steps of 0.1 mm until its box (get_voxel's
    rule, as U.members_np) holds n >= at_least rows of `cloud` with n % block == residue: the box loses rows on its inner face and gains none,
    so n falls through the integers one by one.  Returns (centre [3] fp32, n)."""
    xyz = np.asarray(cloud[:, :3], dtype=np.float32)
    half = np.asarray(size, dtype=np.float32) / np.float32(2)
    c = np.asarray(start, dtype=np.float32).copy()
    lo, hi = (c - half).astype(np.float32), (c + half).astype(np.float32)
    xs = np.sort(xyz[((xyz[:, 1:] >= lo[1:]) & (xyz[:, 1:] <= hi[1:])).all(1), 0])
    cx = (c[0] - np.arange(1, 25000, dtype=np.float32) * np.float32(0.0001)).astype(np.float32)
    n = np.searchsorted(xs, (cx + half[0]).astype(np.float32), "right") - np.searchsorted(xs, (cx - half[0]).astype(np.float32), "left")
    hit = np.nonzero((n >= at_least) & (n % block == residue))[0]
    if not len(hit):
        raise AssertionError(f"no centre beyond {start} whose box holds k * {block} + {residue} rows")
    c[0] = cx[hit[0]]
    return c, int(n[hit[0]])


def special_centres(cloud_1, block):
    """[3, 3] fp32 centres of final boxes of the synthetic scene: one with an exact multiple of `block` rows of cloud_1, one with a multiple
    plus one, one ordinary grid centre; and the two special counts."""
    grid = U.centers_np()
    a, na = centre_with_count(cloud_1, grid[4], U.FINAL, block, 0, U.N_SAMPLES)
    b, nb = centre_with_count(cloud_1, grid[8], U.FINAL, block, 1, U.N_SAMPLES)
    return np.stack([a, b, grid[6]]).astype(np.float32), (na, nb)


def clamp_infs_f64(t):
    """test_flow.py:241-247 on a copy: every +-inf becomes the smallest non-inf entry of the whole tensor."""
    t = t.double().clone()
    inf = t.isinf()
    if inf.any():
        t[inf] = t[~inf].min()
    return t


def change_ragged_f64(lp10, offsets, lp00, multiple, hard_cutoff=None):
    """(change [total] fp64, lp10 clamped fp64, thresholds [B] fp64): test_flow.py:249-275 per voxel, voxel k = lp10[offsets[k]:offsets[k + 1]]
    against row k of lp00."""
    l10, l00 = clamp_infs_f64(lp10.cpu()), clamp_infs_f64(lp00.cpu())
    out = torch.zeros_like(l10)
    thr = torch.zeros(l00.shape[0], dtype=torch.float64)
    for k in range(l00.shape[0]):
        a, b = int(offsets[k]), int(offsets[k + 1])
        thr[k] = (l00[k].mean() - multiple * l00[k].std()) if hard_cutoff is None else hard_cutoff
        if b == a:
            continue
        v = l10[a:b]
        scaled = 1.0 - (v - v.min()) / (v.max() - v.min())
        out[a:b] = torch.where(v < thr[k], scaled, torch.zeros_like(v))
    return out, l10, thr
