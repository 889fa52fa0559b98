"""Input staging, the step right before the log-prob path: farthest point subsampling and the joint
unit-sphere normalisation of the voxel loader (dataloaders/ams_voxel_loader.py:298-307,357-358; utils.py:259-280).

`fps` has the call shape of torch_cluster.fps as the loader uses it (torch-cluster==1.5.9 in the reference's environment.yml;
the package is not in this image, so its published algorithm is restated: start at index 0, squared distances over ALL
columns, first maximum wins).  `unit_sphere` / `co_unit_sphere` mirror utils.py.  All arithmetic runs in the HIP library.
"""
import math
import numbers

import torch

from . import engine


def fps(src, batch=None, ratio=0.5, random_start=True):
    """Indices of the farthest-point subsample of src [n, C] (or a batch of equal-sized clouds given by `batch`)."""
    if random_start:
        raise NotImplementedError("fps: only random_start=False (the loader's setting, ams_voxel_loader.py:298-307) is built")
    if src.dim() != 2:
        raise RuntimeError(f"fps: src must be [n, C], got {tuple(src.shape)}")
    n_total = src.shape[0]
    B = 1
    if batch is not None and batch.numel() > 0:
        B = int(batch.max().item()) + 1
        counts = torch.bincount(batch.to(torch.long), minlength=B)
        if not bool((counts == counts[0]).all()) or not bool((batch[1:] >= batch[:-1]).all()):
            raise NotImplementedError("fps: batches must be sorted and of equal size")
    n = n_total // B
    m = int(math.ceil(ratio * n))
    idx = engine.stage_fps(src.reshape(B, n, src.shape[1]), m)
    return (idx + torch.arange(B, device=idx.device)[:, None] * n).reshape(-1)


def unit_sphere(points, return_inverse=False):
    """utils.py:259-269 (zero mean, unit ball), in place like the reference."""
    empty = points[:0]
    out, _, inv = engine.stage_co_unit_sphere(points.unsqueeze(0), empty.unsqueeze(0))
    points.copy_(out[0])
    if return_inverse:
        return points, {'furthest_distance': inv[0, 0], 'mean': inv[0, 1:4]}
    return points


def co_unit_sphere(points_0, points_1, return_inverse=False):
    """utils.py:271-280: joint zero-mean unit-ball normalisation of a cloud pair."""
    o0, o1, inv = engine.stage_co_unit_sphere(points_0.unsqueeze(0), points_1.unsqueeze(0))
    if return_inverse:
        return o0[0], o1[0], {'furthest_distance': inv[0, 0], 'mean': inv[0, 1:4]}
    return o0[0], o1[0]


def stage_pair(voxel_0_large, voxel_1_small, n_samples_context, n_samples):
    """The loader's last steps for one (context, target) voxel pair: FPS both clouds to their sample counts
    (ams_voxel_loader.py:298-307), then `last_processing` = co_unit_sphere (:357-358)."""
    def sub(v, k):
        sel = fps(v, torch.zeros(v.shape[0], dtype=torch.long, device=v.device), ratio=k / v.shape[0], random_start=False)
        return v[sel][:k]
    return co_unit_sphere(sub(voxel_0_large, n_samples_context), sub(voxel_1_small, n_samples), return_inverse=True)


# ---------------------------------------------------------------- whole scene pairs (csrc/scene_stage.hip)
class SceneStage:
    """What `stage_scene` returns: the staged voxel pairs of a scene, K' valid voxels out of K centres.
    extract_0 [K', M, C], extract_1 [K', N, C], extra_context [K', 1] or None, inverse {'furthest_distance' [K'], 'mean' [K', 3]},
    index_0 [K', M] / index_1 [K', N] (rows of cloud_0 / cloud_1), voxel [K'] (which centres), count_0 / count_1 [K] int32,
    context_counts [K'] int32 (stage_scene's min_context: the context samples of every staged voxel, what inner_loop's `context_counts` takes;
    extract_0[k, count:] is exact zeros and index_0[k, count:] is -1) or None, target_counts [K'] int32 (stage_scene's min_target: the same for
    extract_1 / index_1, what inner_loop's `target_counts` takes) or None."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def batch(self):
        """(extract_0, extract_1, extra_context): what inner_loop takes."""
        return self.extract_0, self.extract_1, self.extra_context


def _scene_input(name, *tensors):
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2):
            raise RuntimeError(f"{name}: expects contiguous float32 [rows, columns] tensors on the GPU (flowcompare_amd has no CPU fallback)")


def _cloud_and_centers(name, cloud, centers):
    _scene_input(name, cloud, centers)
    if not 3 <= cloud.shape[1] <= 8 or cloud.shape[0] < 1 or centers.shape[1] != 3 or centers.device != cloud.device:
        raise RuntimeError(f"{name}: cloud must be [P >= 1, 3..8], centers [K, 3] on the same device; got {tuple(cloud.shape)}, {tuple(centers.shape)}")


def _dims(size):
    d = [float(v) for v in (size.tolist() if torch.is_tensor(size) else size)]
    if len(d) != 3:
        raise RuntimeError("voxel size must be three numbers")
    return d


def voxel_centers(start, end, size, device=None):
    """Centre grid of utils.get_all_voxel_centers / utils.voxelize (utils.py:436-451): arange(start + size/2, end + size/2, size) per
    axis in fp32, x fastest -> [K, 3]."""
    start, end, size = (torch.as_tensor(v, dtype=torch.float32).cpu() for v in (start, end, size))
    axes = [torch.arange(start[i] + size[i] / 2, end[i] + size[i] / 2, size[i]) for i in range(len(size))]
    centers = torch.cartesian_prod(*axes[::-1]).reshape(-1, len(size)).flip(-1).contiguous()
    return centers if device is None else centers.to(device)


def _count(name, cloud, centers, size):
    _cloud_and_centers(name, cloud, centers)
    if centers.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int32, device=cloud.device), None
    return engine.stage_voxel_count(cloud, centers, _dims(size))


def voxel_counts(cloud, centers, size):
    """Points of cloud [P, C] inside every box of `size` around centers [K, 3], utils.get_voxel's rule (utils.py:135-142: both bounds
    inclusive, fp32) -> [K] int32."""
    return _count("voxel_counts", cloud, centers, size)[0]


def _rows(name, cloud, centers, size):
    counts, ws = _count(name, cloud, centers, size)
    offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=cloud.device)
    torch.cumsum(counts, 0, out=offsets[1:])
    total = int(offsets[-1])                                           # the one read-back: sizes `rows`
    rows = engine.stage_voxel_select(cloud, centers, _dims(size), offsets, total, ws) if total else \
        torch.zeros(0, dtype=torch.int32, device=cloud.device)
    return counts, offsets, rows


def voxel_rows(cloud, centers, size):
    """CSR member lists of every box: (offsets [K + 1], rows [total]) int64; rows[offsets[k]:offsets[k + 1]] are the rows of `cloud`
    inside box k in ascending order (= torch.nonzero of get_voxel's mask).  Same input, same bytes on every run."""
    _, offsets, rows = _rows("voxel_rows", cloud, centers, size)
    return offsets, rows.long()


def _fps_ragged(cloud, offsets, rows32, m, voxel_ids=None):
    n = offsets[1:] - offsets[:-1]
    if voxel_ids is not None:
        n = n[voxel_ids.long()]
    if n.numel() == 0:
        return torch.zeros(0, m, dtype=torch.int64, device=cloud.device)
    lo, hi = (int(v) for v in torch.stack((n.min(), n.max())).tolist())
    if m < 1 or lo < m:
        raise RuntimeError(f"fps_ragged: {m} samples asked of a voxel with {lo} rows")
    return engine.stage_fps_ragged(cloud, offsets, rows32, m, hi, None if voxel_ids is None else voxel_ids.to(torch.int32).contiguous())


def _fps_ragged_counts(cloud, offsets, rows32, m, voxel_ids=None):
    """(idx [K', m], sample_counts [K'] int32): voxel v takes min(n_v, m) picks, -1 behind them (engine.stage_fps_ragged_counts).  One
    read-back, the largest voxel, where _fps_ragged reads the smallest and the largest."""
    n = offsets[1:] - offsets[:-1]
    if voxel_ids is not None:
        n = n[voxel_ids.long()]
    if n.numel() == 0:
        return torch.zeros(0, m, dtype=torch.int64, device=cloud.device), torch.zeros(0, dtype=torch.int32, device=cloud.device)
    if m < 1:
        raise RuntimeError(f"fps_ragged_counts: {m} samples asked")
    return engine.stage_fps_ragged_counts(cloud, offsets, rows32, m, int(n.max()), None if voxel_ids is None else voxel_ids.to(torch.int32).contiguous())


def _check_rows(name, cloud, offsets, rows):
    _scene_input(name, cloud)
    if not (offsets.is_cuda and rows.is_cuda and offsets.dtype == torch.int64 and rows.dtype in (torch.int64, torch.int32)):
        raise RuntimeError(f"{name}: offsets (int64) and rows must be GPU tensors (flowcompare_amd has no CPU fallback)")
    if not 1 <= cloud.shape[1] <= 8:
        raise RuntimeError(f"{name}: 1..8 feature columns supported")
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= cloud.shape[0]) or int(offsets[-1]) != rows.numel():
        raise RuntimeError(f"{name}: rows / offsets do not describe rows of this cloud")


def fps_ragged_counts(cloud, offsets, rows, m, voxel_ids=None):
    """fps_ragged for voxels that may hold fewer than m rows -> (idx [K', m] int64, sample_counts [K'] int32): voxel v with n_v rows takes
    m_v = min(n_v, m) picks; idx[v, :m_v] are the picks of `fps(cloud[rows of voxel v], random_start=False)` with m_v samples, index for
    index, idx[v, m_v:] is -1 and sample_counts[v] = m_v (0 for a voxel without rows).  voxel_ids [K'] (optional): which voxels of the CSR
    list, in that order, repeats allowed; None = all of them."""
    _check_rows("fps_ragged_counts", cloud, offsets, rows)
    if voxel_ids is not None:
        if not (torch.is_tensor(voxel_ids) and voxel_ids.is_cuda and voxel_ids.dim() == 1 and voxel_ids.dtype in (torch.int64, torch.int32)):
            raise RuntimeError("fps_ragged_counts: voxel_ids must be a 1-d integer GPU tensor")
        if voxel_ids.numel() and (int(voxel_ids.min()) < 0 or int(voxel_ids.max()) >= offsets.numel() - 1):
            raise RuntimeError("fps_ragged_counts: voxel_ids name voxels outside the list")
    return _fps_ragged_counts(cloud, offsets.contiguous(), rows.to(torch.int32).contiguous(), int(m), voxel_ids)


def fps_ragged(cloud, offsets, rows, m):
    """Farthest point subsampling of every voxel of a CSR list (voxel_rows) in one launch -> [K, m] int64 rows of `cloud`: the first m
    picks of `fps(cloud[rows of voxel k], random_start=False)`, index for index.  Raises if a voxel has fewer than m rows."""
    _scene_input("fps_ragged", cloud)
    if not (offsets.is_cuda and rows.is_cuda and offsets.dtype == torch.int64 and rows.dtype in (torch.int64, torch.int32)):
        raise RuntimeError("fps_ragged: offsets (int64) and rows must be GPU tensors (flowcompare_amd has no CPU fallback)")
    if not 1 <= cloud.shape[1] <= 8:
        raise RuntimeError("fps_ragged: 1..8 feature columns supported")
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= cloud.shape[0] or int(offsets[-1]) != rows.numel()):
        raise RuntimeError("fps_ragged: rows / offsets do not describe rows of this cloud")
    return _fps_ragged(cloud, offsets.contiguous(), rows.to(torch.int32).contiguous(), int(m))


def _min_context(name, min_context, M):
    """min_context of stage_scene / scene_change: None, or a plain integer in [1, n_samples_context]."""
    if min_context is None:
        return None
    if isinstance(min_context, bool) or torch.is_tensor(min_context) or not isinstance(min_context, numbers.Integral):
        raise RuntimeError(f"{name}: min_context must be None or an integer, got {type(min_context).__name__}")
    if not 1 <= min_context <= M:
        raise RuntimeError(f"{name}: min_context must lie in [1, n_samples_context = {M}], got {int(min_context)}")
    return int(min_context)


def _min_target(name, min_target, N, lowest=1, why=""):
    """min_target of stage_scene / scene_change: None, or a plain integer in [lowest, n_samples]."""
    if min_target is None:
        return None
    if isinstance(min_target, bool) or torch.is_tensor(min_target) or not isinstance(min_target, numbers.Integral):
        raise RuntimeError(f"{name}: min_target must be None or an integer, got {type(min_target).__name__}")
    if not lowest <= min_target <= N:
        raise RuntimeError(f"{name}: min_target must lie in [{lowest}, n_samples = {N}], got {int(min_target)}{why}")
    return int(min_target)


def stage_scene(cloud_0, cloud_1, centers, final_voxel_size, context_voxel_size, n_samples, n_samples_context, ground_height=None, min_context=None,
                min_target=None):
    """The loader's test-mode item (ams_voxel_loader.py:291-307, 338, 349-350) for every centre of a scene at once: target =
    get_voxel(cloud_1, c, final) -> first n_samples FPS picks, context = get_voxel(cloud_0, c, context) -> first n_samples_context
    picks, co_unit_sphere(context, target).  A voxel is valid when count_0 >= n_samples_context and count_1 >= n_samples (:240);
    invalid voxels are skipped, never padded; staged voxels keep ascending centre order.  Returns a SceneStage; with no valid voxel
    its tensors are empty and nothing is launched beyond the counts.  stage_scene(cloud_0, cloud_0, ...) is the "self" pair.

    min_context (an integer in [1, n_samples_context]) keeps voxels with sparse context: a voxel is valid when count_0 >=
    min_context and count_1 >= n_samples, and valid voxel k gets min(count_0[k], n_samples_context) context samples -- its rows are bit for bit
    stage_pair(cloud_0[members], cloud_1[members], that count, n_samples); extract_0[k, count:] is exact zeros, index_0[k, count:] is -1, and
    SceneStage.context_counts [K'] int32 holds the counts: st.batch() plus context_counts=st.context_counts is what inner_loop takes.  The
    target side is untouched by min_context (min_target, below, gives it a count of its own).  With None nothing changes and context_counts is None.

    min_target (an integer in [1, n_samples]) does the same for the target: a voxel is valid when count_1 >= min_target (the
    context rule is whatever min_context makes it), valid voxel k gets n_k = min(count_1[k], n_samples) target samples, extract_1[k, n_k:] is exact
    zeros, index_1[k, n_k:] is -1, SceneStage.target_counts [K'] int32 holds the n_k, and the pair is bit for bit stage_pair on the truncated
    clouds.  min_target = n_samples gives the tensors of None (plus the counts); with None target_counts is None."""
    _cloud_and_centers("stage_scene", cloud_0, centers)
    _cloud_and_centers("stage_scene", cloud_1, centers)
    if cloud_0.shape[1] != cloud_1.shape[1] or cloud_0.device != cloud_1.device:
        raise RuntimeError("stage_scene: the two clouds must have the same columns and device")
    M, N, C, dev = int(n_samples_context), int(n_samples), cloud_0.shape[1], cloud_0.device
    if M < 1 or N < 1:
        raise RuntimeError("stage_scene: sample counts must be positive")
    min_context = _min_context("stage_scene", min_context, M)
    min_target = _min_target("stage_scene", min_target, N)
    count_0, ws_0 = _count("stage_scene", cloud_0, centers, context_voxel_size)
    count_1, ws_1 = _count("stage_scene", cloud_1, centers, final_voxel_size)
    voxel = torch.nonzero((count_0 >= (M if min_context is None else min_context)) & (count_1 >= (N if min_target is None else min_target))).flatten()
    K1 = voxel.numel()
    if K1 == 0:
        f, i = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
        return SceneStage(extract_0=torch.zeros(0, M, C, **f), extract_1=torch.zeros(0, N, C, **f),
                          extra_context=None if ground_height is None else torch.zeros(0, 1, **f),
                          inverse={'furthest_distance': torch.zeros(0, **f), 'mean': torch.zeros(0, 3, **f)},
                          index_0=torch.zeros(0, M, **i), index_1=torch.zeros(0, N, **i), voxel=voxel, count_0=count_0, count_1=count_1,
                          context_counts=None if min_context is None else torch.zeros(0, dtype=torch.int32, device=dev),
                          target_counts=None if min_target is None else torch.zeros(0, dtype=torch.int32, device=dev))

    def picks(cloud, size, counts, ws, m, ragged=_fps_ragged):
        offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=offsets[1:])
        rows = engine.stage_voxel_select(cloud, centers, _dims(size), offsets, int(offsets[-1]), ws)
        return ragged(cloud, offsets, rows, m, voxel)

    target_counts = None
    if min_target is not None:                                         # a count on both sides; counts_0 None = every context row real
        index_0, context_counts = picks(cloud_0, context_voxel_size, count_0, ws_0, M, _fps_ragged_counts) if min_context is not None else \
            (picks(cloud_0, context_voxel_size, count_0, ws_0, M), None)
        index_1, target_counts = picks(cloud_1, final_voxel_size, count_1, ws_1, N, _fps_ragged_counts)
        o0, o1, inv = engine.stage_pairs_counts2(cloud_0, cloud_1, index_0, index_1, context_counts, target_counts)
    elif min_context is None:
        context_counts = None
        index_0 = picks(cloud_0, context_voxel_size, count_0, ws_0, M)
        index_1 = picks(cloud_1, final_voxel_size, count_1, ws_1, N)
        e0 = cloud_0.index_select(0, index_0.reshape(-1)).reshape(K1, M, C)
        e1 = cloud_1.index_select(0, index_1.reshape(-1)).reshape(K1, N, C)
        o0, o1, inv = engine.stage_co_unit_sphere(e0, e1)
    else:                                                              # index_0 holds -1 behind a sparse voxel's count: the pair kernel reads through the lists
        index_0, context_counts = picks(cloud_0, context_voxel_size, count_0, ws_0, M, _fps_ragged_counts)
        index_1 = picks(cloud_1, final_voxel_size, count_1, ws_1, N)
        o0, o1, inv = engine.stage_pairs_counts(cloud_0, cloud_1, index_0, index_1, context_counts)
    inverse = {'furthest_distance': inv[:, 0].contiguous(), 'mean': inv[:, 1:4].contiguous()}
    extra = None if ground_height is None else (inverse['mean'][:, 2] - ground_height).unsqueeze(-1)
    return SceneStage(extract_0=o0, extract_1=o1, extra_context=extra, inverse=inverse, index_0=index_0, index_1=index_1, voxel=voxel,
                      count_0=count_0, count_1=count_1, context_counts=context_counts, target_counts=target_counts)


# ---------------------------------------------------------------- every member of the staged voxels (csrc/scene_stage.hip)
class DenseStage:
    """What `stage_dense` returns: ALL members of the K' staged voxels, packed into blocks of `block` rows.
    blocks [n_blocks, block, C] (normalised like the sample), index [n_blocks, block] int64 (row of the cloud, -1 in pad slots),
    block_voxel [n_blocks] int32 (which staged voxel), offsets [K' + 1] / rows [total] int64 (the CSR member lists of the staged voxels),
    block_offsets [K' + 1] int64 (first block of every voxel), block.  Masking a per-slot result with `index >= 0` leaves it in CSR order."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def stage_dense(cloud, st, final_voxel_size, centers, block):
    """All members of every voxel that `st` (a SceneStage of stage_scene(..., cloud, centers, final_voxel_size, ...)) staged, as
    engine-shaped batches: voxel i = centre centers[st.voxel[i]] owns ceil(count / block) consecutive blocks holding its member rows of
    `cloud` in ascending order, xyz normalised with the SAMPLE's mean and furthest_distance (st.inverse) by the operations of
    co_unit_sphere, other columns as they are.  A member that is also an FPS pick has the same bits as in st.extract_1.  The slots of a
    voxel's last block beyond its count repeat the voxel's first member (index -1).  furthest_distance comes from the sample, so dense
    points can lie slightly OUTSIDE the unit ball.  The member lists are voxel_rows'; one read-back sizes the blocks.  Returns a
    DenseStage; for an empty `st` its tensors are empty and nothing is launched."""
    _cloud_and_centers("stage_dense", cloud, centers)
    block = int(block)
    if block < 1:
        raise RuntimeError(f"stage_dense: block must be at least 1, got {block}")
    K1, dev, C = st.voxel.numel(), cloud.device, cloud.shape[1]
    if st.count_1.numel() != centers.shape[0] or st.extract_1.shape[0] != K1 or st.inverse["mean"].shape[0] != K1 or st.extract_1.shape[2] != C:
        raise RuntimeError(f"stage_dense: the SceneStage does not belong to these centres: it counted {st.count_1.numel()} centres and staged "
                           f"{st.extract_1.shape[0]} voxels of {st.extract_1.shape[2]} columns, given are {centers.shape[0]} centres and {C} columns")
    i64 = dict(dtype=torch.int64, device=dev)
    if K1 == 0:
        return DenseStage(blocks=torch.zeros(0, block, C, dtype=torch.float32, device=dev), index=torch.zeros(0, block, **i64),
                          block_voxel=torch.zeros(0, dtype=torch.int32, device=dev), offsets=torch.zeros(1, **i64), rows=torch.zeros(0, **i64),
                          block_offsets=torch.zeros(1, **i64), block=block)
    sel = centers.index_select(0, st.voxel).contiguous()
    counts, offsets, rows32 = _rows("stage_dense", cloud, sel, final_voxel_size)
    block_offsets = torch.zeros(K1 + 1, **i64)
    torch.cumsum((counts.long() + (block - 1)) // block, 0, out=block_offsets[1:])
    same = (counts == st.count_1.index_select(0, st.voxel)).all()
    n_blocks, same = torch.stack((block_offsets[-1], same.long())).tolist()       # the one read-back: sizes the blocks
    if not same:
        raise RuntimeError("stage_dense: the voxels' member counts differ from the SceneStage's count_1: another cloud, centres or box size")
    inverse = torch.cat((st.inverse["furthest_distance"].reshape(K1, 1), st.inverse["mean"].reshape(K1, 3)), 1).contiguous()
    blocks, index, block_voxel = engine.stage_dense_blocks(cloud, offsets, rows32, inverse, block_offsets, n_blocks, block)
    return DenseStage(blocks=blocks, index=index, block_voxel=block_voxel, offsets=offsets, rows=rows32.long(), block_offsets=block_offsets,
                      block=block)
