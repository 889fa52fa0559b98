"""Change maps of voxels with few target points (include/fcflow_sparse_target.h, csrc/scene_stage.hip, csrc/staging.hip)
on the GPU.  Every comparison has an existing entry on its other side: the pair kernel against staging.stage_pair on the truncated pair and
engine.stage_pairs_counts, the counted change maps against change.log_prob_to_change on truncated rows and engine.change_map /
change_map_ragged, stage_scene(min_target) against stage_pair per voxel and the numpy restatement of tests/sparse_target_util.py,
inner_loop(target_counts=) against the same call without counts, and scene_change / scene_context_attribution with min_target against their
hand-written compositions.  The scene is the fixture scene in its own direction: target = the thinned cloud, whose 32 final boxes hold 89, 103
and 678 .. 767 points (pinned in tests/test_sparse_target_host.py), M = 1024, N = 720."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

import flowcompare_amd as fa
import scene_stage_util as U
import sparse_target_util as TU
from flowcompare_amd import change, engine, staging

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, N, MT = TU.M, TU.N, TU.MIN_TARGET
NAN = float("nan")


def _same(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(-1.0), b.nan_to_num(-1.0))


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def _csr(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=DEV)


# ---------------------------------------------------------------- 1. the pair kernel
def _pairs2_raw(c0, c1, i0, i1, n0, n1, ld=None):
    """fc_stage_pairs_counts2_f32 on NaN-filled outputs -> (out_0, out_1, inverse)"""
    (K, m), n, C = i0.shape, i1.shape[1], c0.shape[1]
    o0, o1, inv = (torch.full(s, NAN, device=DEV) for s in ((K, m, C), (K, n, C), (K, 4)))
    engine.lib().fc_stage_pairs_counts2_f32(engine._ptr(c0), c0.shape[0], engine._ptr(c1), c1.shape[0], C if ld is None else ld, engine._ptr(i0),
                                            engine._ptr(i1), engine._ptr(n0), engine._ptr(n1), K, m, n, engine._ptr(o0), engine._ptr(o1),
                                            engine._ptr(inv), engine._stream())
    torch.cuda.synchronize()
    return o0, o1, inv


def _hand_made_pairs(m, n, counts, seed):
    """clouds [P, 6] and lists as the ragged FPS writes them for voxels of exactly the wanted sizes: (cloud_0, cloud_1, index_0 [K, m], index_1
    [K, n], member rows per pair).  The voxels' rows are random, not contiguous, and overlap."""
    g = torch.Generator().manual_seed(seed)
    c0, c1 = torch.rand(3000, 6, generator=g).to(DEV) * 4 - 1, torch.rand(2500, 6, generator=g).to(DEV) * 4 + 0.5
    rows_0 = [torch.randperm(3000, generator=g)[:c].sort().values.to(DEV) for c, _ in counts]
    rows_1 = [torch.randperm(2500, generator=g)[:k].sort().values.to(DEV) for _, k in counts]
    i0, k0 = staging.fps_ragged_counts(c0, _csr([c for c, _ in counts]), torch.cat(rows_0), m)
    i1, k1 = staging.fps_ragged_counts(c1, _csr([k for _, k in counts]), torch.cat(rows_1), n)
    assert k0.tolist() == [c for c, _ in counts] and k1.tolist() == [k for _, k in counts]
    return c0, c1, i0, i1, rows_0, rows_1


def _check_pairs(m, n, counts, seed):
    c0, c1, i0, i1, rows_0, rows_1 = _hand_made_pairs(m, n, counts, seed)
    n0, n1 = _i32([c for c, _ in counts]), _i32([k for _, k in counts])
    o0, o1, inv = _pairs2_raw(c0, c1, i0, i1, n0, n1)
    for k, (c, t) in enumerate(counts):
        s0, s1, ref = staging.stage_pair(c0[rows_0[k]], c1[rows_1[k]], c, t)      # the existing single-pair path on the truncated pair
        assert torch.equal(o0[k, :c], s0) and torch.equal(o1[k, :t], s1), (m, n, c, t)
        assert torch.equal(inv[k, 0], ref["furthest_distance"]) and torch.equal(inv[k, 1:4], ref["mean"]), (m, n, c, t)
        assert bool((o0[k, c:] == 0).all()) and bool((o1[k, t:] == 0).all()), (m, n, c, t)         # exact zeros, from NaN-filled outputs
        assert bool((i0[k, c:] == -1).all()) and bool((i1[k, t:] == -1).all())
    assert bool(torch.isfinite(o0).all()) and bool(torch.isfinite(o1).all()) and bool(torch.isfinite(inv).all())
    # what stands behind a count in the lists is never read: -1 (above), far outside the clouds, or a valid row -- the same bytes
    col_m, col_n = torch.arange(m, device=DEV)[None, :], torch.arange(n, device=DEV)[None, :]
    for junk in (2 ** 40, -(2 ** 40), 7):
        j0, j1 = torch.where(col_m < n0[:, None], i0, junk), torch.where(col_n < n1[:, None], i1, junk)
        p0, p1, pinv = _pairs2_raw(c0, c1, j0, j1, n0, n1)
        assert torch.equal(p0, o0) and torch.equal(p1, o1) and torch.equal(pinv, inv), junk
    e0, e1, einv = engine.stage_pairs_counts2(c0, c1, i0, i1, n0, n1)
    assert torch.equal(e0, o0) and torch.equal(e1, o1) and torch.equal(einv, inv)
    return c0, c1, i0, i1, n0, n1, (o0, o1, inv)


def test_pair_kernel_equals_stage_pair_on_the_truncated_pair():
    _check_pairs(40, 33, [(40, 33), (40, 1), (1, 33), (17, 32), (1, 1)], seed=1)


def test_pair_kernel_around_the_stride_of_its_loops():
    """c + n = 1023, 1024, 1025: the last pass of the 1024-thread loops holds 1023 rows, a full pass, one row of a second pass"""
    counts = [(959, 64), (960, 64), (961, 64), (1000, 23), (1000, 24), (1000, 25)]
    c0, c1, i0, i1, n0, n1, (o0, o1, inv) = _check_pairs(1000, 64, counts, seed=2)
    assert sorted(c + n for c, n in counts) == [1023, 1023, 1024, 1024, 1025, 1025]
    # counts_0 null = every context row real
    full = [k for k, (c, _) in enumerate(counts) if c == 1000]
    z0, z1, zinv = _pairs2_raw(c0, c1, i0[full].contiguous(), i1[full].contiguous(), None, n1[full].contiguous())
    assert torch.equal(z0, o0[full]) and torch.equal(z1, o1[full]) and torch.equal(zinv, inv[full])
    y0, y1, yinv = engine.stage_pairs_counts2(c0, c1, i0[full].contiguous(), i1[full].contiguous(), None, n1[full].contiguous())
    assert torch.equal(y0, z0) and torch.equal(y1, z1) and torch.equal(yinv, zinv)


def test_pair_kernel_with_full_target_counts_equals_the_existing_entry():
    counts = [(40, 33), (1, 33), (17, 33), (39, 33)]
    c0, c1, i0, i1, rows_0, rows_1 = _hand_made_pairs(40, 33, counts, seed=3)
    n0 = _i32([c for c, _ in counts])
    a0, a1, ainv = engine.stage_pairs_counts(c0, c1, i0, i1, n0)
    for n1 in (_i32([33] * 4), _i32([34, 1000, 33, 2 ** 31 - 1])):                 # counts above N are clamped
        b0, b1, binv = _pairs2_raw(c0, c1, i0, i1, n0, n1)
        assert torch.equal(a0, b0) and torch.equal(a1, b1) and torch.equal(ainv, binv)
    # counts below 1 are clamped to 1, never an out-of-range read
    z0, z1, _ = _pairs2_raw(c0, c1, i0, i1, _i32([0, -5, 0, 0]), _i32([0, 0, -1, 0]))
    assert bool((z0[:, 1:] == 0).all()) and bool((z1[:, 1:] == 0).all()) and bool(torch.isfinite(z0).all()) and bool(torch.isfinite(z1).all())


def test_pair_kernel_refusals_launch_nothing():
    c0, c1, i0, i1, _, _ = _hand_made_pairs(8, 4, [(8, 4), (3, 2)], seed=4)
    n0, n1 = _i32([8, 3]), _i32([4, 2])

    def untouched(outs):
        torch.cuda.synchronize()
        return all(bool(o.isnan().all()) for o in outs)

    lib, p, s = engine.lib(), engine._ptr, engine._stream
    for what, args in (("null pointer", dict(n1=None)), ("null pointer", dict(c1=None)), ("3..8 columns", dict(ld=9)), ("3..8 columns", dict(ld=2)),
                       ("bad sample counts", dict(n=0)), ("bad sample counts", dict(m=0)), ("bad cloud size", dict(P0=0)),
                       ("bad argument", dict(K=-1))):
        a = dict(c0=c0, c1=c1, n0=n0, n1=n1, ld=6, m=8, n=4, P0=c0.shape[0], K=2)
        a.update(args)
        outs = [torch.full(sh, NAN, device=DEV) for sh in ((2, 8, 6), (2, 4, 6), (2, 4))]
        with pytest.raises(engine.FcError, match=what):
            lib.fc_stage_pairs_counts2_f32(p(a["c0"]), a["P0"], p(a["c1"]), c1.shape[0], a["ld"], p(i0), p(i1), p(a["n0"]), p(a["n1"]), a["K"], a["m"], a["n"],
                                           p(outs[0]), p(outs[1]), p(outs[2]), s())
        assert untouched(outs), what
    for bad in (dict(counts_1=n1.long()), dict(counts_1=n1[:1]), dict(counts_1=n1.cpu()), dict(index_1=i1.int()), dict(counts_0=n0.float())):
        a = dict(cloud_0=c0, cloud_1=c1, index_0=i0, index_1=i1, counts_0=n0, counts_1=n1)
        a.update(bad)
        with pytest.raises(RuntimeError, match="stage_pairs_counts2"):
            engine.stage_pairs_counts2(**a)


# ---------------------------------------------------------------- 2. the change map with a length per row on both sides
B, NC = 6, 300
C1 = [2, 255, 256, 257, 300, 300]                                                 # around the 256-thread stride, on either side
C0 = [300, 257, 2, 256, 255, 2]


def _log_probs(seed, pads="random"):
    """(lp10 [B, NC], lp00 [B, NC]) with the given pad values behind C1 / C0; real slots depend on the seed only"""
    g = torch.Generator().manual_seed(seed)
    lp10, lp00 = torch.randn(B, NC, generator=g) * 3 - 5, torch.randn(B, NC, generator=g) * 2 - 3
    col = torch.arange(NC)[None, :]
    for t, cnt in ((lp10, C1), (lp00, C0)):
        pad = col >= torch.tensor(cnt)[:, None]
        if pads == "poison":                                                      # -inf and a huge negative value, alternating
            t[pad] = torch.where(torch.arange(int(pad.sum())) % 2 == 0, float("-inf"), -1e30)
        elif pads == "nan":
            t[pad] = NAN
    return lp10.to(DEV), lp00.to(DEV)


def _rows_by_the_existing_entry(lp10, lp00, c1, c0, multiple, cutoff):
    """row b = log_prob_to_change(lp10[b:b+1, :n1], lp00[b:b+1, :n0]) on copies; NaN behind n1"""
    out = torch.full_like(lp10, NAN)
    for b, (n1, n0) in enumerate(zip(c1, c0)):
        out[b, :n1] = change.log_prob_to_change(lp10[b:b + 1, :n1].clone(), lp00[b:b + 1, :n0].clone(), multiple, cutoff)[0]
    return out


@pytest.mark.parametrize("multiple, cutoff", [(1.0, None), (0.5, -6.0)])
def test_change_map_counts_rows_equal_the_existing_entry_on_truncated_rows(multiple, cutoff):
    lp10, lp00 = _log_probs(5)
    ref = _rows_by_the_existing_entry(lp10, lp00, C1, C0, multiple, cutoff)
    keep10, keep00 = lp10.clone(), lp00.clone()
    out = change.log_prob_to_change_counts(lp10, _i32(C1), lp00, _i32(C0), multiple, cutoff)
    assert _same(out, ref) and bool((out[:, :2] >= 0).all()) and bool((out.nan_to_num(0.0) > 0).any())
    col = torch.arange(NC, device=DEV)[None, :]
    assert torch.equal(out.isnan(), col >= _i32(C1)[:, None])                      # output pads are NaN, real slots finite
    assert torch.equal(lp10, keep10) and torch.equal(lp00, keep00)                # no inf: nothing is clamped
    # pad values change nothing, and pads of the inputs stay as they were
    for pads in ("poison", "nan"):
        p10, p00 = _log_probs(5, pads)
        k10, k00 = p10.clone(), p00.clone()
        with contextlib.redirect_stdout(io.StringIO()) as said:
            again = change.log_prob_to_change_counts(p10, _i32(C1), p00, _i32(C0), multiple, cutoff)
        assert _same(again, out), pads
        assert _same(p10, k10) and _same(p00, k00) and said.getvalue() == "", pads          # not clamped, not reported: no REAL slot held an inf
    # counts as int64 are taken too; counts_0 None = all of N0
    none = change.log_prob_to_change_counts(lp10, torch.tensor(C1, device=DEV), lp00, None, multiple, cutoff)
    assert _same(none, _rows_by_the_existing_entry(lp10, lp00, C1, [NC] * B, multiple, cutoff))


def test_change_map_counts_clamps_infs_over_real_slots_only():
    lp10, lp00 = _log_probs(6, "poison")
    lp10[1, 100], lp10[4, 299], lp00[0, 17], lp00[3, 255] = float("-inf"), float("inf"), float("-inf"), float("-inf")        # real slots
    col = torch.arange(NC, device=DEV)[None, :]
    real1, real0 = col < _i32(C1)[:, None], col < _i32(C0)[:, None]
    # clamp_infs by hand: the minimum over the REAL non-inf slots of each tensor (the pads' -1e30 must not feed it)
    m1, m0 = lp10[real1 & ~lp10.isinf()].min(), lp00[real0 & ~lp00.isinf()].min()
    assert float(m1) > -40 and float(m0) > -40
    e10, e00 = torch.where(real1 & lp10.isinf(), m1, lp10), torch.where(real0 & lp00.isinf(), m0, lp00)
    ref = _rows_by_the_existing_entry(e10, e00, C1, C0, 1.0, None)
    with contextlib.redirect_stdout(io.StringIO()) as said:
        out = change.log_prob_to_change_counts(lp10, _i32(C1), lp00, _i32(C0), 1.0)
    assert _same(out, ref) and "Clamping infs!" in said.getvalue()
    assert _same(lp10, e10) and _same(lp00, e00)                                  # real infs clamped in place, pads as they were
    assert bool(lp10[~real1].isinf().any()) and bool((lp10[~real1] == -1e30).any())


def test_change_map_counts_full_counts_give_the_bytes_of_the_existing_entry():
    for plant in (False, True):
        lp10, lp00 = _log_probs(7)
        if plant:
            lp10[2, 5], lp00[4, 200] = float("-inf"), float("inf")
        a10, a00, b10, b00 = lp10.clone(), lp00.clone(), lp10.clone(), lp00.clone()
        ref, bad = engine.change_map(a10, a00, 1.0)
        for c0 in (_i32([NC] * B), None, _i32([NC + 7] * B)):
            out, bad2 = engine.change_map_counts(b10, _i32([NC] * B), b00, c0, 1.0)
            assert torch.equal(out, ref) and bad2 == bad is False and torch.equal(a10, b10) and torch.equal(a00, b00)


def test_change_map_counts_baseline_of_one_value():
    lp10, lp00 = _log_probs(8)
    c0 = [300, 257, 1, 256, 255, 2]
    lp10[0, 0], lp00[0, 3] = float("-inf"), float("inf")                          # real slots of another scene
    keep10, keep00 = lp10.clone(), lp00.clone()
    with pytest.raises(RuntimeError, match=r"change_map_counts: scene 2 has a baseline of 1 value\(s\): without hard_cutoff .*unbiased std needs two"):
        change.log_prob_to_change_counts(lp10, _i32(C1), lp00, _i32(c0), 1.0)
    assert torch.equal(lp10, keep10) and torch.equal(lp00, keep00)                # refused before the launch: nothing was clamped
    lp10, lp00 = _log_probs(8)
    out = change.log_prob_to_change_counts(lp10, _i32(C1), lp00, _i32(c0), 1.0, hard_cutoff=-6.0)      # with a hard cutoff the baseline is not used
    assert _same(out, _rows_by_the_existing_entry(lp10, lp00, C1, c0, 1.0, -6.0))
    for bad in (dict(counts_1=_i32(C1)[:3]), dict(counts_1=torch.tensor(C1)), dict(counts_1=_i32(C1).float()), dict(counts_0=_i32(C0)[:5])):
        a = dict(counts_1=_i32(C1), counts_0=_i32(C0))
        a.update(bad)
        with pytest.raises(RuntimeError, match="log_prob_to_change_counts"):
            change.log_prob_to_change_counts(lp10, a["counts_1"], lp00, a["counts_0"], 1.0)
    with pytest.raises(RuntimeError, match="change_map_counts"):
        engine.change_map_counts(lp10, _i32(C1).long(), lp00, None, 1.0)


def test_ragged_change_map_with_base_counts():
    sizes = [5, 300, 0, 257, 1000, 64]
    off = _csr(sizes)
    g = torch.Generator().manual_seed(9)
    flat = (torch.randn(sum(sizes), generator=g) * 3 - 5).to(DEV)
    _, lp00 = _log_probs(9, "poison")
    keep00 = lp00.clone()
    for multiple, cutoff in ((1.0, None), (0.5, -6.0)):
        out = change.log_prob_to_change_ragged(flat, off, lp00, multiple, cutoff, base_counts=_i32(C0))
        for b, n in enumerate(sizes):
            if n:
                lo = int(off[b])
                ref = change.log_prob_to_change(flat[lo:lo + n].clone()[None], lp00[b:b + 1, :C0[b]].clone(), multiple, cutoff)[0]
                assert torch.equal(out[lo:lo + n], ref), (b, n)
        assert _same(lp00, keep00)                                                # the pads' -inf was neither seen nor clamped
    # an inf in a real slot of either tensor: clamped over real slots, in place
    f2, l2 = flat.clone(), lp00.clone()
    f2[400], l2[1, 3] = float("-inf"), float("-inf")
    real0 = torch.arange(NC, device=DEV)[None, :] < _i32(C0)[:, None]
    m1, m0 = f2[~f2.isinf()].min(), l2[real0 & ~l2.isinf()].min()
    e1, e0 = torch.where(f2.isinf(), m1, f2), torch.where(real0 & l2.isinf(), m0, l2)
    with contextlib.redirect_stdout(io.StringIO()):
        out = change.log_prob_to_change_ragged(f2, off, l2, 1.0, base_counts=_i32(C0))
    assert torch.equal(f2, e1) and _same(l2, e0)
    for b, n in enumerate(sizes):
        if n:
            lo = int(off[b])
            assert torch.equal(out[lo:lo + n], change.log_prob_to_change(e1[lo:lo + n].clone()[None], e0[b:b + 1, :C0[b]].clone(), 1.0)[0]), b
    # full counts / None: the bytes of the existing entry
    _, clean = _log_probs(9)
    ref, _ = engine.change_map_ragged(flat.clone(), off, clean.clone(), 1.0)
    for c0 in (_i32([NC] * B), None):
        got, bad = engine.change_map_ragged(flat.clone(), off, clean.clone(), 1.0, counts_0=c0)
        assert torch.equal(got, ref) and not bad
    one = [300, 257, 2, 1, 255, 2]
    f3, c3 = flat.clone(), clean.clone()
    f3[1] = float("-inf")
    k3 = f3.clone()
    with pytest.raises(RuntimeError, match=r"change_map_ragged: scene 3 has a baseline of 1 value\(s\): without"):
        change.log_prob_to_change_ragged(f3, off, c3, 1.0, base_counts=_i32(one))
    assert torch.equal(f3, k3) and torch.equal(c3, clean)                         # refused before the launch: nothing was clamped
    # a voxel without rows contributes nothing, whatever its baseline length: voxel 2 with a baseline of 1 value, no hard cutoff
    empty_short = [300, 257, 1, 256, 255, 2]
    got = change.log_prob_to_change_ragged(flat.clone(), off, clean.clone(), 1.0, base_counts=_i32(empty_short))
    assert torch.equal(got, change.log_prob_to_change_ragged(flat.clone(), off, clean.clone(), 1.0, base_counts=_i32(C0)))
    assert change.log_prob_to_change_ragged(flat, off, clean, 1.0, hard_cutoff=-6.0, base_counts=_i32(one)).shape == flat.shape
    with pytest.raises(RuntimeError, match="base_counts"):
        change.log_prob_to_change_ragged(flat, off, clean, 1.0, base_counts=_i32(one)[:2])


# ---------------------------------------------------------------- 3. stage_scene(min_target)
@pytest.fixture(scope="module")
def scene():
    c0, c1 = U.scene()
    return torch.from_numpy(c0).to(DEV), torch.from_numpy(c1).to(DEV), torch.from_numpy(U.centers_np()).to(DEV)


@pytest.fixture(scope="module")
def staged(scene):
    c0, c1, centers = scene
    return staging.stage_scene(c0, c1, centers, U.FINAL, U.CONTEXT, N, M, ground_height=U.GROUND, min_target=MT)


FIELDS = ("extract_0", "extract_1", "extra_context", "index_0", "index_1", "voxel", "count_0", "count_1")


def _same_stage(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in FIELDS) and all(torch.equal(a.inverse[k], b.inverse[k]) for k in a.inverse)


def test_stage_scene_with_min_target_equals_stage_pair_per_voxel(scene, staged):
    c0, c1, centers = scene
    st = staged
    o0, r0 = staging.voxel_rows(c0, centers, U.CONTEXT)
    o1, r1 = staging.voxel_rows(c1, centers, U.FINAL)
    assert st.voxel.tolist() == list(range(32)) and st.target_counts.dtype == torch.int32 and st.target_counts.is_cuda and st.context_counts is None
    assert torch.equal(st.target_counts, st.count_1.clamp(max=N)) and st.extract_1.shape == (32, N, 6) and st.index_1.shape == (32, N)
    counts = st.target_counts.tolist()
    assert sum(n < N for n in counts) == 13 and sorted(counts)[:3] == [89, 103, 678]
    for k, n in enumerate(counts):
        s0, s1, inv = staging.stage_pair(c0[r0[o0[k]:o0[k + 1]]], c1[r1[o1[k]:o1[k + 1]]], M, n)
        assert torch.equal(st.extract_0[k], s0) and torch.equal(st.extract_1[k, :n], s1), (k, n)
        assert torch.equal(st.inverse["furthest_distance"][k], inv["furthest_distance"]) and torch.equal(st.inverse["mean"][k], inv["mean"]), k
        assert torch.equal(st.extra_context[k], (inv["mean"][2] - U.GROUND).unsqueeze(-1))
        assert bool((st.extract_1[k, n:] == 0).all()) and bool((st.index_1[k, n:] == -1).all()) and bool((st.index_1[k, :n] >= 0).all()), k
        assert torch.equal(c1[st.index_1[k, :n]][:, 3:], st.extract_1[k, :n, 3:])
    again = staging.stage_scene(c0, c1, centers, U.FINAL, U.CONTEXT, N, M, ground_height=U.GROUND, min_target=MT)
    assert _same_stage(st, again) and torch.equal(st.target_counts, again.target_counts)                # same input, same bytes


def test_stage_scene_with_min_target_against_the_numpy_restatement(staged):
    st = staged
    n0, n1 = U.scene()
    r = TU.stage_target_np(n0, n1, U.centers_np(), U.FINAL, U.CONTEXT, N, M, MT)
    assert st.voxel.tolist() == r["voxel"].tolist() and st.target_counts.tolist() == r["target_counts"].tolist()
    assert np.array_equal(st.count_0.cpu().numpy(), r["count_0"]) and np.array_equal(st.count_1.cpu().numpy(), r["count_1"])
    differ = 0
    for i in range(32):
        i0, i1 = st.index_0[i].cpu().numpy(), st.index_1[i].cpu().numpy()
        if not (np.array_equal(i0, r["index_0"][i]) and np.array_equal(i1, r["index_1"][i])):
            n = int(r["target_counts"][i])                                        # an fp64 tie of the FPS: tests/test_gpu_sparse_stage.py's rule
            TU.assert_fp64_tie(i0, r["index_0"][i], n0, f"voxel {i} index_0")
            TU.assert_fp64_tie(i1[:n], r["index_1"][i][:n], n1, f"voxel {i} index_1")
            differ += 1
            continue
        e0 = np.abs(st.extract_0[i].cpu().numpy() - r["extract_0"][i]).max()
        e1 = np.abs(st.extract_1[i].cpu().numpy() - r["extract_1"][i]).max()
        assert e0 < 1e-6 and e1 < 1e-6, (i, e0, e1)
        assert abs(float(st.inverse["furthest_distance"][i]) - float(r["far"][i])) < 1e-4
        assert np.abs(st.inverse["mean"][i].cpu().numpy() - r["mean"][i]).max() < 1e-5
    print(f"voxels whose selection differs from the numpy restatement: {differ}")
    assert differ <= 1


def test_min_target_values(scene, staged, monkeypatch):
    c0, c1, centers = scene
    args = (c0, c1, centers, U.FINAL, U.CONTEXT, N, M)
    today = staging.stage_scene(*args, ground_height=U.GROUND)
    assert today.target_counts is None and today.voxel.numel() == 19
    at_n = staging.stage_scene(*args, ground_height=U.GROUND, min_target=N)
    assert _same_stage(today, at_n) and at_n.target_counts.tolist() == [N] * 19 and bool((at_n.index_1 >= 0).all())
    st96 = staging.stage_scene(*args, min_target=96)
    assert st96.voxel.tolist() == list(range(31)) and st96.extra_context is None and int(st96.target_counts.min()) == 103
    assert torch.equal(st96.extract_1, staged.extract_1[:31]) and torch.equal(st96.index_1, staged.index_1[:31])
    empty = staging.stage_scene(c0, c1, centers + 1000.0, U.FINAL, U.CONTEXT, N, M, min_target=MT)
    assert empty.voxel.numel() == 0 and empty.target_counts.shape == (0,) and empty.target_counts.dtype == torch.int32
    # with min_context: the swapped scene, cloud 0 the target (711 .. 817 points per final box), per voxel stage_pair on both truncated clouds
    n, m = 750, 1280
    both = staging.stage_scene(c1, c0, centers[12:18].contiguous(), U.FINAL, U.CONTEXT, n, m, min_context=256, min_target=700)
    assert both.voxel.tolist() == list(range(6)) and bool((both.context_counts < m).any()) and bool((both.target_counts < n).any())
    o0, r0 = staging.voxel_rows(c1, centers[12:18].contiguous(), U.CONTEXT)
    o1, r1 = staging.voxel_rows(c0, centers[12:18].contiguous(), U.FINAL)
    for k, (c, t) in enumerate(zip(both.context_counts.tolist(), both.target_counts.tolist())):
        s0, s1, inv = staging.stage_pair(c1[r0[o0[k]:o0[k + 1]]], c0[r1[o1[k]:o1[k + 1]]], c, t)
        assert torch.equal(both.extract_0[k, :c], s0) and torch.equal(both.extract_1[k, :t], s1) and torch.equal(both.inverse["mean"][k], inv["mean"])
        assert bool((both.extract_0[k, c:] == 0).all()) and bool((both.extract_1[k, t:] == 0).all())
        assert bool((both.index_0[k, c:] == -1).all()) and bool((both.index_1[k, t:] == -1).all())
    ctx_only = staging.stage_scene(c1, c0, centers[12:18].contiguous(), U.FINAL, U.CONTEXT, n, m, min_context=256)
    keep = torch.tensor([k in ctx_only.voxel.tolist() for k in range(6)], device=DEV)
    assert 0 < int(keep.sum()) < 6 and torch.equal(ctx_only.extract_0, both.extract_0[keep]) and torch.equal(ctx_only.extract_1, both.extract_1[keep])

    def never(*a, **k):
        raise AssertionError("launched before the refusal")
    for name in ("stage_voxel_count", "stage_voxel_select", "stage_fps_ragged", "stage_fps_ragged_counts", "stage_pairs_counts", "stage_pairs_counts2",
                 "stage_co_unit_sphere"):
        monkeypatch.setattr(engine, name, never)
    for bad in (0, N + 1, 2.5, torch.tensor(64, device=DEV)):
        with pytest.raises(RuntimeError, match="min_target must"):
            staging.stage_scene(*args, min_target=bad)


# ---------------------------------------------------------------- 4. inner_loop(target_counts=)
def _model(**kw):
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=2, sample_size=N, n_samples_context=M, **kw)
    cfg["final_voxel_size"], cfg["context_voxel_size"] = U.FINAL, U.CONTEXT
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    return cfg, md


@pytest.fixture(scope="module")
def model():
    return _model()


A, Z = 12, 16                                                                     # the chunk of the tests below: voxels 12 .. 15, voxel 15 holds 103 points


def test_inner_loop_with_target_counts(staged, model):
    cfg, md = model
    st = staged
    cnt = st.target_counts[A:Z]
    assert cnt.tolist()[3] == 103 and int((cnt < N).sum()) >= 2
    g = torch.Generator().manual_seed(3)
    eps = [torch.randn(s, generator=g).to(DEV) for s in md["flow"].noise_shapes(Z - A, N)]
    batch = (st.extract_0[A:Z], st.extract_1[A:Z], st.extra_context[A:Z])
    real = torch.arange(N, device=DEV)[None, :] < cnt[:, None]
    _, plain, _ = fa.inner_loop(batch, md, cfg, eps=eps)                          # the existing call on the zero-padded batch
    fallbacks = engine.lib().fc_debug_fp16_fallbacks()
    loss, lp, bpd = fa.inner_loop(batch, md, cfg, eps=eps, target_counts=cnt)
    assert torch.equal(lp[real], plain[real]) and bool(lp[~real].isnan().all()) and bool(torch.isfinite(lp[real]).all())
    assert torch.equal(loss, -lp[real].mean()) and torch.equal(bpd, loss * math.log2(math.exp(1)) / cfg["input_dim"])
    assert abs(float(loss) + float(plain[real].double().mean())) < 1e-4 * abs(float(loss))
    # whatever the caller's pad rows hold does not reach the flow or its range flag
    for junk in (NAN, 1e30):
        e1 = torch.where(real[:, :, None], st.extract_1[A:Z], junk)
        l2, lp2, _ = fa.inner_loop((batch[0], e1, batch[2]), md, cfg, eps=eps, target_counts=cnt)
        assert _same(lp2, lp) and torch.equal(l2, loss), junk
        assert engine.lib().fc_debug_fp16_fallbacks() == fallbacks, junk
    # int64 counts, and together with context_counts (all full here: the same bytes as context_counts alone)
    full = torch.full((Z - A,), M, dtype=torch.int32, device=DEV)
    _, with_ctx, _ = fa.inner_loop(batch, md, cfg, eps=eps, context_counts=full, target_counts=cnt.long())
    _, ctx_only, _ = fa.inner_loop(batch, md, cfg, eps=eps, context_counts=full)
    assert torch.equal(with_ctx[real], ctx_only[real]) and bool(with_ctx[~real].isnan().all())
    # pad_target_batch builds such a batch
    e1, c = fa.pad_target_batch([st.extract_1[k, :n] for k, n in zip(range(A, Z), cnt.tolist())])
    assert torch.equal(c, cnt) and torch.equal(e1, st.extract_1[A:Z, :int(cnt.max())])
    for bad in (cnt[:2], torch.zeros_like(cnt), cnt + N, cnt.float(), cnt.cpu()):
        with pytest.raises(RuntimeError, match="target_counts"):
            fa.inner_loop(batch, md, cfg, eps=eps, target_counts=bad)


def test_a_thin_voxel_in_a_chunk_scores_as_it_does_alone(staged, model):
    """Pinned eps: voxels 15 (103 target points) and 12 (704) inside its padded chunk against the scene alone on its truncated pair.  The bound is the
    existing path's own row invariance at these shapes, measured first through the existing entry (the zero-padded chunk without counts
    against a row slice of it): torch.equal when that gap is 0.0, otherwise that gap."""
    cfg, md = model
    st = staged
    cnt = st.target_counts[A:Z]
    g = torch.Generator().manual_seed(4)
    eps = [torch.randn(s, generator=g).to(DEV) for s in md["flow"].noise_shapes(Z - A, N)]
    batch = (st.extract_0[A:Z], st.extract_1[A:Z], st.extra_context[A:Z])
    _, plain, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    _, lp, _ = fa.inner_loop(batch, md, cfg, eps=eps, target_counts=cnt)
    for k in (15, 12):
        n, j = int(st.target_counts[k]), k - A
        one = (st.extract_0[k:k + 1], st.extract_1[k:k + 1, :n].contiguous(), st.extra_context[k:k + 1])
        _, alone, _ = fa.inner_loop(one, md, dict(cfg, sample_size=n), eps=[e[j:j + 1, :n].contiguous() for e in eps])
        gap = (plain[j:j + 1, :n] - alone).abs().max().item()                     # existing entry against existing entry
        d = (lp[j:j + 1, :n] - alone).abs().max().item()
        print(f"voxel {k} ({n} target points): existing path, chunk of {Z - A} x {N} against its slice 1 x {n}: max |d| {gap:.3e}; with target_counts {d:.3e}")
        assert bool(torch.isfinite(alone).all())
        if gap == 0.0:
            assert torch.equal(lp[j:j + 1, :n], alone), (k, d)
        else:
            assert d <= gap, (k, d, gap)


def test_target_counts_refuse_train_mode_and_a_sharded_models_dict(staged):
    cfg, md = _model()
    st = staged
    batch = (st.extract_0[A:Z], st.extract_1[A:Z], st.extra_context[A:Z])
    with pytest.raises(RuntimeError, match="inner_loop: target_counts is not supported with a sharded models_dict"):
        fa.inner_loop(batch, dict(md, sharded=True), cfg, target_counts=st.target_counts[A:Z])
    md["flow"].train()
    with pytest.raises(RuntimeError, match="inner_loop: target_counts is eval-mode only"):
        fa.inner_loop(batch, md, cfg, target_counts=st.target_counts[A:Z])
    c0 = c1 = centers = None                                                      # refused before a cloud is looked at
    with pytest.raises(RuntimeError, match="scene_change: min_target is eval-mode only"):
        fa.scene_change(c0, c1, md, cfg, centers, ground_height=U.GROUND, min_target=MT)
    with pytest.raises(RuntimeError, match="scene_context_attribution: min_target is eval-mode only"):
        fa.scene_context_attribution(c0, c1, md, cfg, centers, ground_height=U.GROUND, min_target=MT)
    md["flow"].eval()
    with pytest.raises(RuntimeError, match="scene_change: min_target must lie in .*unbiased std"):
        fa.scene_change(c0, c1, md, cfg, centers, ground_height=U.GROUND, min_target=1)


# ---------------------------------------------------------------- 5. scene_change, sampled and dense, and scene_context_attribution
KW = dict(ground_height=U.GROUND, multiple=1.0, voxels_per_batch=7)           # multiple = 1: some points of every voxel are marked


def _by_hand_stagings(scene):
    c0, c1, centers = scene
    ok = (staging.voxel_counts(c0, centers, U.CONTEXT) >= M) & (staging.voxel_counts(c1, centers, U.FINAL) >= MT) & \
        (staging.voxel_counts(c0, centers, U.FINAL) >= MT)
    assert int(ok.sum()) == 32
    sel = centers[ok].contiguous()
    s10 = staging.stage_scene(c0, c1, sel, U.FINAL, U.CONTEXT, N, M, U.GROUND, min_target=MT)
    s00 = staging.stage_scene(c0, c0, sel, U.FINAL, U.CONTEXT, N, M, U.GROUND, min_target=MT)
    assert torch.equal(s10.index_0, s00.index_0) and not torch.equal(s10.target_counts, s00.target_counts)
    assert int((s00.target_counts < N).sum()) == 3 and int(s00.target_counts.min()) == 711
    return sel, s10, s00


def _thin_members(scene):
    """rows of cloud 1 inside the two thinned final boxes (voxels 15 and 31)"""
    _, c1, centers = scene
    off, rows = staging.voxel_rows(c1, centers, U.FINAL)
    return torch.cat([rows[off[k]:off[k + 1]] for k in (15, 31)])


def test_scene_change_with_min_target_equals_the_hand_written_composition(scene, model):
    c0, c1, centers = scene
    cfg, md = model
    torch.manual_seed(11)
    out, st = fa.scene_change(c0, c1, md, cfg, centers, min_target=MT, **KW)
    torch.manual_seed(11)
    out_none, st_none = fa.scene_change(c0, c1, md, cfg, centers, **KW)
    torch.manual_seed(11)
    out_n, st_n = fa.scene_change(c0, c1, md, cfg, centers, min_target=N, **KW)
    assert st_none.target_counts is None and st_none.voxel.numel() == 17
    assert _same(out_n, out_none) and torch.equal(st_n.index_1, st_none.index_1) and st_n.target_counts.tolist() == [N] * 17

    sel, s10, s00 = _by_hand_stagings(scene)
    torch.manual_seed(11)
    chunks = []
    for a in range(0, 32, 7):
        ex, t10, t00 = s10.extra_context[a:a + 7], s10.target_counts[a:a + 7], s00.target_counts[a:a + 7]
        _, l10, _ = fa.inner_loop((s10.extract_0[a:a + 7], s10.extract_1[a:a + 7], ex), md, cfg, target_counts=t10)
        _, l00, _ = fa.inner_loop((s00.extract_0[a:a + 7], s00.extract_1[a:a + 7], ex), md, cfg, target_counts=t00)
        chunks.append(change.log_prob_to_change_counts(l10, t10, l00, t00, 1.0))
    flat, vals = s10.index_1.reshape(-1), torch.cat(chunks).reshape(-1)
    assert torch.equal(vals.isnan(), flat < 0)                                    # NaN exactly in the pad slots
    ref = torch.full((c1.shape[0],), NAN, device=DEV)
    ref.scatter_reduce_(0, flat[flat >= 0], vals[flat >= 0], "amax", include_self=False)
    assert _same(out, ref)
    touched = torch.zeros(c1.shape[0], dtype=torch.bool, device=DEV)
    touched[flat[flat >= 0]] = True
    assert torch.equal(torch.isfinite(out), touched) and torch.equal(out.isnan(), ~touched)
    assert float(out[touched].min()) >= 0.0 and float(out[touched].max()) <= 1.0 and bool((out[touched] > 0).any())
    assert torch.equal(st.index_1, s10.index_1) and torch.equal(st.target_counts, s10.target_counts) and st.voxel.tolist() == list(range(32))
    # what it buys: the two thinned boxes, where the scene really changed, are scored; strictly more points evaluated, none lost
    thin = _thin_members(scene)
    assert thin.numel() == 103 + 89 and bool(torch.isfinite(out[thin]).all()) and bool(out_none[thin].isnan().all())
    fin, fin_none = torch.isfinite(out), torch.isfinite(out_none)
    assert int(fin.sum()) > int(fin_none.sum()) > 0 and bool(fin[fin_none].all())
    print(f"sampled: {int(fin_none.sum())} points scored without min_target, {int(fin.sum())} with min_target = {MT}")


def test_dense_scene_change_with_min_target(scene, model):
    c0, c1, centers = scene
    cfg, md = model
    torch.manual_seed(11)
    out, st = fa.scene_change(c0, c1, md, cfg, centers, dense=True, block=256, min_target=MT, **KW)
    torch.manual_seed(11)
    out_none, _ = fa.scene_change(c0, c1, md, cfg, centers, dense=True, block=256, **KW)
    torch.manual_seed(11)
    out_n, _ = fa.scene_change(c0, c1, md, cfg, centers, dense=True, block=256, min_target=N, **KW)
    assert _same(out_n, out_none)

    sel, s10, s00 = _by_hand_stagings(scene)
    dense = staging.stage_dense(c1, s10, U.FINAL, sel, 256)
    torch.manual_seed(11)
    l10 = fa.dense_log_prob(s10, dense, md, cfg, blocks_per_batch=7)
    l00 = torch.cat([fa.inner_loop((s00.extract_0[a:a + 7], s00.extract_1[a:a + 7], s10.extra_context[a:a + 7]), md, cfg,
                                   target_counts=s00.target_counts[a:a + 7])[1] for a in range(0, 32, 7)])
    assert l10.shape == (dense.rows.numel(),) and l00.shape == (32, N) and int(l00.isnan().sum()) == int((N - s00.target_counts.long()).sum()) > 0
    vals = change.log_prob_to_change_ragged(l10, dense.offsets, l00, 1.0, base_counts=s00.target_counts)
    ref = torch.full((c1.shape[0],), NAN, device=DEV)
    ref.scatter_reduce_(0, dense.rows, vals, "amax", include_self=False)
    assert _same(out, ref)
    assert torch.equal(st.dense.index, dense.index) and torch.equal(st.target_counts, s10.target_counts)
    touched = torch.zeros(c1.shape[0], dtype=torch.bool, device=DEV)
    touched[dense.rows] = True
    assert torch.equal(torch.isfinite(out), touched) and torch.equal(out.isnan(), ~touched)
    assert float(out[touched].min()) >= 0.0 and float(out[touched].max()) <= 1.0 and bool((out[touched] > 0).any())
    thin = _thin_members(scene)
    assert bool(torch.isfinite(out[thin]).all()) and bool(out_none[thin].isnan().all())
    # a thin voxel's members are all picked: its dense rows are its sample
    for k in (15, 31):
        n = int(s10.target_counts[k])
        lo, hi = int(dense.offsets[k]), int(dense.offsets[k + 1])
        assert hi - lo == n and sorted(dense.rows[lo:hi].tolist()) == sorted(s10.index_1[k, :n].tolist())
    fin, fin_none = torch.isfinite(out), torch.isfinite(out_none)
    assert int(fin.sum()) > int(fin_none.sum()) > 0 and bool(fin[fin_none].all())
    print(f"dense: {int(fin_none.sum())} points scored without min_target, {int(fin.sum())} with min_target = {MT}")


@pytest.mark.parametrize("weight", ["change", "uniform"])
def test_scene_context_attribution_with_min_target(scene, weight):
    c0, c1, centers = scene
    cfg, md = _model(latent_dim=16, cif_latent_dim=16)
    layers = ["aug", 1]
    torch.manual_seed(11)
    mass_0, change_1, st = fa.scene_context_attribution(c0, c1, md, cfg, centers, layers=layers, min_target=MT, weight=weight, **KW)
    assert tuple(mass_0.shape) == (2, c0.shape[0]) and tuple(change_1.shape) == (c1.shape[0],)

    sel, s10, s00 = _by_hand_stagings(scene)
    torch.manual_seed(11)
    chunks, masses = [], []
    for a in range(0, 32, 7):
        ex, t10, t00 = s10.extra_context[a:a + 7], s10.target_counts[a:a + 7], s00.target_counts[a:a + 7]
        b10 = (s10.extract_0[a:a + 7], s10.extract_1[a:a + 7], ex)
        eps = [torch.randn(s, device=DEV) for s in md["flow"].noise_shapes(b10[1].shape[0], N)]
        _, a10, _ = fa.inner_loop(b10, md, cfg, eps=eps, target_counts=t10)
        _, a00, _ = fa.inner_loop((s00.extract_0[a:a + 7], s00.extract_1[a:a + 7], ex), md, cfg, eps=eps, target_counts=t00)
        ch = change.log_prob_to_change_counts(a10, t10, a00, t00, 1.0)
        chunks.append(ch)
        real = s10.index_1[a:a + 7] >= 0
        assert torch.equal(ch.isnan(), ~real)
        w = torch.where(real, ch, 0.0) if weight == "change" else real.float()   # weight 0 on the pad slots
        masses.append(torch.stack(fa.attention_mass(b10, md, cfg, layers=layers, weights=w, eps=eps)))
    flat, vals = s10.index_1.reshape(-1), torch.cat(chunks).reshape(-1)
    ref_c = torch.full((c1.shape[0],), NAN, device=DEV)
    ref_c.scatter_reduce_(0, flat[flat >= 0], vals[flat >= 0], "amax", include_self=False)
    ref_m = torch.full((2, c0.shape[0]), NAN, device=DEV)
    allm = torch.cat(masses, dim=1).reshape(2, -1)
    for i in range(2):
        ref_m[i].scatter_reduce_(0, s10.index_0.reshape(-1), allm[i], "amax", include_self=False)
    assert _same(change_1, ref_c) and _same(mass_0, ref_m)
    assert bool(torch.isfinite(change_1[_thin_members(scene)]).all())
    touched = torch.zeros(c0.shape[0], dtype=torch.bool, device=DEV)
    touched[s10.index_0.reshape(-1)] = True
    for i in range(2):
        assert torch.equal(torch.isfinite(mass_0[i]), touched)
    assert float(mass_0[:, touched].min()) >= 0.0 and bool((mass_0[:, touched] > 0).any())
    assert torch.equal(st.index_1, s10.index_1) and torch.equal(st.target_counts, s10.target_counts)
    if weight == "change":                                                        # min_target = N: the call without it
        torch.manual_seed(11)
        m_n, ch_n, _ = fa.scene_context_attribution(c0, c1, md, cfg, centers, layers=layers, min_target=N, weight=weight, **KW)
        torch.manual_seed(11)
        m_none, ch_none, _ = fa.scene_context_attribution(c0, c1, md, cfg, centers, layers=layers, weight=weight, **KW)
        assert _same(ch_n, ch_none) and _same(m_n, m_none)
