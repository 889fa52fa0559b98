"""The DGCNN embedder with per-scene point counts (include/fcflow_embed_counts.h) on the GPU.  Every bit-for-bit
comparison has the existing entries on its other side: the scene alone, as f[b:b+1, :c] / pts[b:b+1, :c].

operator   engine.op_knn(..., counts=) against engine.op_knn(f[b:b+1, :c], k): both kernels, the batch on both sides of the kernel
           threshold, warm starts, full counts, pad rows, refusals;
engine     DgcnnHandle.embed(pts, counts) per point and global, pad rows of pts and of the output;
callers    inner_loop and scene_change embed a ragged batch in ONE pass (gather_max launches), with the results of count_aware = False."""
import contextlib
import functools
import io

import pytest
import torch

import flowcompare_amd as fa
import scene_stage_util as U
import sparse_stage_util as SU
from flowcompare_amd import engine, model_initialization
from knob_util import knobs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77


class _kernels:
    """{kernel name: launches} of the launches inside the block (the helper of tests/test_gpu_context_counts.py)"""

    def __enter__(self):
        engine.profile_stride(1); engine.profile_filter(None); engine.profile_enable(True); engine.profile_reset()
        self.launches = {}
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                torch.cuda.synchronize()
                self.launches = {r["kernel"]: r["launches"] for r in engine.profile_report()}
        finally:
            engine.profile_enable(False); engine.profile_reset()
        return False

    def count(self, substr):
        return sum(n for name, n in self.launches.items() if substr in name)


def _cnt(counts):
    return torch.tensor(counts, dtype=torch.int32, device=DEV)


def _quantised(B, M, C, seed, steps):
    """_quantised of tests/test_gpu_knn_degenerate.py: features on a grid of 1 / steps in [-1, 1], fp32-exact, plenty of exact ties"""
    g = torch.Generator().manual_seed(seed)
    return torch.round((torch.rand(B, M, C, generator=g) * 2 - 1) * steps) / steps


def _features(B, M, C, seed=71):
    return (_quantised(B, M, C, seed, 8) if C == 6 else torch.rand(B, M, C, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV)


def _check_against_alone(got, f, k, counts, what):
    """rows < c of scene b: the cold search of the scene alone; rows >= c: the -1 the binding handed in"""
    for b, c in enumerate(counts):
        alone = engine.op_knn(f[b:b + 1, :c].contiguous(), k)
        assert torch.equal(got[b:b + 1, :c], alone), f"{what}: scene {b} ({c} points) differs from its search alone"
        assert bool((got[b, c:] == -1).all()), f"{what}: scene {b}: rows >= {c} of the index buffer were written"


# ------------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize("counts", [(200, 137, 64, 20), (65, 63, 129, 33)])
@pytest.mark.parametrize("C", [6, 64, 128])
def test_lane_kernel_with_counts_equals_every_scene_alone(C, counts):
    """knob 24 = 0: counts either side of the 64-candidate tile and the 16-query workgroup, and count = k"""
    B, M, k = 4, 200, 20
    f = _features(B, M, C)
    with knobs({24: 0}):
        with _kernels() as kn:
            got = engine.op_knn(f, k, counts=_cnt(counts))
        assert kn.count("knn_counts_kernel") == 1 and kn.count("knn_mfma") == 0 and kn.count("fc::knn_kernel") == 0, kn.launches
        _check_against_alone(got, f, k, counts, f"lane kernel, C = {C}")


@pytest.mark.parametrize("counts", [(200, 129, 128, 127), (65, 64, 33, 20)])
@pytest.mark.parametrize("C", [6, 64, 128])
def test_mfma_kernel_with_counts_cold_warm_and_in_place(C, counts):
    """knob 24 = 2: counts round the 128-query workgroup, the 64-candidate block and its 32-candidate tiles; cold, warm from the sets of a
    perturbed cloud, and warm in place all equal the cold search of the scene alone"""
    B, M, k = 4, 200, 20
    f = _features(B, M, C)
    cnt = _cnt(counts)
    with knobs({24: 2}):
        with _kernels() as kn:
            cold = engine.op_knn(f, k, counts=cnt)
        assert kn.count("knn_mfma_counts_kernel") == 1 and kn.count("knn_counts_kernel") == 0 and kn.count("knn_mfma_kernel") == 0, kn.launches
        _check_against_alone(cold, f, k, counts, f"mfma kernel cold, C = {C}")
        g = torch.Generator().manual_seed(72)
        warm = engine.op_knn(f + 0.1 * torch.randn(B, M, C, generator=g).to(DEV), k, counts=cnt)
        _check_against_alone(engine.op_knn(f, k, warm=warm, counts=cnt), f, k, counts, f"mfma kernel warm, C = {C}")
        keep = warm.clone()
        _check_against_alone(engine.op_knn(f, k, warm=warm, in_place=True, counts=cnt), f, k, counts, f"mfma kernel warm in place, C = {C}")
        assert torch.equal(warm, keep)


STRADDLE = (2100, 2048, 2047, 40)


@functools.lru_cache(maxsize=None)
def _straddle_alone(C):
    """the searches alone of the straddling batch: scenes 0 and 1 on the matrix cores, 2 and 3 on the lane kernel (computed once per C)"""
    f = _features(4, 2100, C)
    alone = []
    for b, c in enumerate(STRADDLE):
        with _kernels() as kn:
            alone.append(engine.op_knn(f[b:b + 1, :c].contiguous(), 40))
        assert (kn.count("knn_mfma_kernel"), kn.count("fc::knn_kernel")) == ((1, 0) if c >= 2048 else (0, 1)), (c, kn.launches)
    return f, alone


@pytest.mark.parametrize("C", [6, 64])
def test_a_batch_that_straddles_the_kernel_boundary(C):
    """shipped knob, M = 2100: one launch of each kernel, and every scene gets the sets of the kernel it takes alone"""
    f, alone = _straddle_alone(C)
    with _kernels() as kn:
        got = engine.op_knn(f, 40, counts=_cnt(STRADDLE))
    assert kn.count("knn_counts_kernel") == 1 and kn.count("knn_mfma_counts_kernel") == 1, kn.launches
    for b, c in enumerate(STRADDLE):
        assert torch.equal(got[b:b + 1, :c], alone[b]), f"scene {b} ({c} points)"
        assert bool((got[b, c:] == -1).all())
    with _kernels() as kn:
        engine.op_knn(f, 40, counts=_cnt((2047, 300, 64, 40)))
    assert kn.count("knn_counts_kernel") == 1 and kn.count("knn_mfma") == 0, kn.launches
    with _kernels() as kn:
        full_side = engine.op_knn(f, 40, counts=_cnt((2100, 2048, 2048, 2100)))
    assert kn.count("knn_mfma_counts_kernel") == 1 and kn.count("knn_counts_kernel") == 0, kn.launches
    assert torch.equal(full_side[0:1], alone[0]) and torch.equal(full_side[1:2, :2048], alone[1])


@pytest.mark.parametrize("knob24", [0, 2])
def test_full_counts_and_pad_rows_of_the_features(knob24):
    B, M, C, k = 4, 200, 64, 20
    f = _features(B, M, C)
    counts = (200, 137, 64, 20)
    cnt = _cnt(counts)
    pad = torch.arange(M, device=DEV)[None, :, None] >= cnt[:, None, None]
    with knobs({24: knob24}):
        assert torch.equal(engine.op_knn(f, k, counts=_cnt([M] * B)), engine.op_knn(f, k)), "full counts: the bytes of the uniform call"
        zeros = engine.op_knn(f.masked_fill(pad, 0.0), k, counts=cnt)
        for fill in (float("nan"), 1e30):
            assert torch.equal(engine.op_knn(f.masked_fill(pad, fill), k, counts=cnt), zeros), fill


@pytest.mark.parametrize("knob24", [0, 2])
@pytest.mark.parametrize("lo,hi,null,code,message", [
    (19, 200, False, 1, "fewer points than neighbours"), (20, 201, False, 1, "k <= count_min <= count_max <= M"),
    (100, 64, False, 1, "k <= count_min <= count_max <= M"), (20, 200, True, 1, "null counts"),
])
def test_refusals_return_their_status_and_launch_nothing(lo, hi, null, code, message, knob24):
    B, M, C, k = 4, 200, 6, 20
    f = torch.zeros(B, M, C, device=DEV)
    cnt = _cnt((200, 137, 64, 20))
    idx = torch.full((B, M, k), SENTINEL, dtype=torch.int32, device=DEV)
    L = engine.lib()
    with knobs({24: knob24}):
        with _kernels() as kn:
            with pytest.raises(engine.FcError, match=message) as e:
                L.fc_op_knn_counts_f32(engine._ptr(f), None, None if null else engine._ptr(cnt), lo, hi, engine._ptr(idx), B, M, C, k, engine._stream())
    assert e.value.code == code
    assert kn.launches == {}, f"a refused search launched {kn.launches}"
    assert bool((idx == SENTINEL).all()), "a refused search wrote to its output"


def test_binding_refuses_bad_counts_by_message():
    f = torch.zeros(4, 200, 6, device=DEV)
    for bad, message in ((_cnt([200, 137, 64]), r"counts must have shape \[B\] with B = 4"), (_cnt([200, 137, 64, 0]), r"counts out of range: count 0"),
                         (_cnt([201, 137, 64, 20]), r"counts out of range: count 201"), (_cnt([200, 137, 64, 20]).float(), "counts must be an integer tensor"),
                         (_cnt([200, 137, 64, 20]).cpu(), "counts must live on a HIP device")):
        with pytest.raises(RuntimeError, match=message):
            engine.op_knn(f, 20, counts=bad)
    with pytest.raises(engine.FcError, match="fewer points than neighbours"):
        engine.op_knn(f, 20, counts=_cnt([200, 137, 64, 19]))


# ------------------------------------------------------------------------------------------------ engine
@functools.lru_cache(maxsize=None)
def _stack(name, N=130, **kw):
    """Two layers of a named configuration, built like _stack of tests/test_gpu_context_counts.py"""
    cfg = fa.named_config(name, n_flow_layers=2, sample_size=N, **kw)
    torch.manual_seed(7)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    return cfg, md


def _clouds(B, M, C, seed):
    return torch.rand(B, M, C, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _gaps(handle, pts, counts):
    """(uniform gap, counted gap, counted result, scenes alone): the B-scene uniform call against its B = 1 calls through the existing entry,
    and the counted call against the scenes alone on their own rows"""
    B = pts.shape[0]
    uniform = handle.embed(pts)
    uni_gap = max((uniform[b:b + 1] - handle.embed(pts[b:b + 1])).abs().max().item() for b in range(B))
    got = handle.embed(pts, counts=_cnt(counts))
    alone = [handle.embed(pts[b:b + 1, :c].contiguous()) for b, c in enumerate(counts)]
    cut = (lambda b, c: got[b:b + 1]) if handle.is_global else (lambda b, c: got[b:b + 1, :c])
    gap = max((cut(b, c) - alone[b]).abs().max().item() for b, c in enumerate(counts))
    return uni_gap, gap, got, alone, uniform


def _by_the_rule(uni_gap, gap, equal, what):
    """the convention of test_inner_loop_with_counts_and_pad_context_batch: bit for bit where the uniform path is batch-invariant on this
    input, otherwise no further from the scenes alone than the uniform batch is"""
    print(f"{what}: uniform batch against its scenes alone max |d| {uni_gap:.2e}; counted batch against its scenes alone {gap:.2e}")
    if uni_gap == 0.0:
        assert equal(), what
    else:
        assert gap <= uni_gap, what


@pytest.mark.parametrize("M,counts", [(200, (200, 137, 64, None)), (2100, (2100, 2048, 2047, 40))], ids=["M200", "M2100"])
def test_per_point_handle_with_counts_equals_every_scene_alone(M, counts):
    cfg, md = _stack("c2_dgcnn_attn_spline")
    handle = md["input_embedder"]._engine()
    counts = tuple(cfg["n_neighbors"] if c is None else c for c in counts)
    pts = _clouds(4, M, 6, 21)
    with torch.no_grad():
        uni_gap, gap, got, alone, uniform = _gaps(handle, pts, counts)
        _by_the_rule(uni_gap, gap, lambda: all(torch.equal(got[b:b + 1, :c], alone[b]) for b, c in enumerate(counts)), f"per-point embed, M = {M}")
        # output rows >= c are exactly 0, from a buffer the test prefilled with NaN
        out = torch.full_like(got, float("nan"))
        assert handle.embed(pts, counts=_cnt(counts), out=out) is out and torch.equal(out, got)
        for b, c in enumerate(counts):
            assert bool((got[b, c:] == 0).all()) and bool(torch.isfinite(got[b]).all())
        assert torch.equal(handle.embed(pts, counts=_cnt([M] * 4)), uniform), "full counts: the bytes of the uniform call"
        # count_range from a caller that has read the counts back: the same bytes
        assert torch.equal(handle.embed(pts, counts=_cnt(counts), count_range=(min(counts), max(counts))), got)


def test_pad_rows_of_the_points_do_not_matter():
    cfg, md = _stack("c2_dgcnn_attn_spline")
    handle = md["input_embedder"]._engine()
    counts = (200, 137, 64, cfg["n_neighbors"])
    cnt = _cnt(counts)
    pts = _clouds(4, 200, 6, 22)
    pad = torch.arange(200, device=DEV)[None, :, None] >= cnt[:, None, None]
    lib = engine.lib()
    with torch.no_grad():
        zeros = handle.embed(pts.masked_fill(pad, 0.0), counts=cnt)
        assert torch.equal(handle.embed(pts, counts=cnt), zeros)
        before = lib.fc_debug_fp16_fallbacks()
        for fill in (float("nan"), 1e30):
            got = handle.embed(pts.masked_fill(pad, fill), counts=cnt)
            assert bool(torch.isfinite(got).all()) and torch.equal(got, zeros), fill
        assert lib.fc_debug_fp16_fallbacks() == before


def test_global_handle_with_counts_equals_every_scene_alone():
    cfg, md = _stack("c1_dgcnn_global_affine")
    handle = md["input_embedder"]._engine()
    assert handle.is_global
    counts = (200, 137, 64, cfg["n_neighbors"])
    pts = _clouds(4, 200, cfg["input_dim"], 23)
    with torch.no_grad():
        uni_gap, gap, got, alone, uniform = _gaps(handle, pts, counts)
        assert tuple(got.shape) == (4, handle.out_dim)
        _by_the_rule(uni_gap, gap, lambda: torch.equal(got, torch.cat(alone)), "global embed")
        assert torch.equal(handle.embed(pts, counts=_cnt([200] * 4)), uniform)
        pad = torch.arange(200, device=DEV)[None, :, None] >= _cnt(counts)[:, None, None]
        assert torch.equal(handle.embed(pts.masked_fill(pad, float("nan")), counts=_cnt(counts)), got)


def test_handles_refuse_by_message():
    cfg, md = _stack("c2_dgcnn_attn_spline")
    handle = md["input_embedder"]._engine()
    k = cfg["n_neighbors"]
    pts = _clouds(4, 200, 6, 24)
    with pytest.raises(engine.FcError, match=r"fewer context points than n_neighbors \(torch.topk raises in the reference\)"):
        handle.embed(pts, counts=_cnt((200, 137, 64, k - 1)))
    with pytest.raises(RuntimeError, match=r"counts must have shape \[B\] with B = 4"):
        handle.embed(pts, counts=_cnt((200, 137, 64)))
    with pytest.raises(RuntimeError, match=r"counts out of range: count 201 is not in \[1, 200\]"):
        handle.embed(pts, counts=_cnt((200, 137, 64, k)), count_range=(k, 201))
    out = torch.full((4, 200, handle.out_dim), float(SENTINEL), device=DEV)
    ws = torch.empty(1 << 26, dtype=torch.uint8, device=DEV)
    for lo, hi, null, message in ((k, 201, False, "count_min <= count_max <= M"), (100, 64, False, "count_min <= count_max <= M"), (k, 200, True, "null counts")):
        with _kernels() as kn:
            with pytest.raises(engine.FcError, match=message):
                engine.lib().fc_dgcnn_embed_counts_f32(handle._h, engine._ptr(pts), None if null else engine._ptr(_cnt((200, 137, 64, k))), lo, hi, engine._ptr(out),
                                                      4, 200, engine._ptr(ws), ws.numel(), engine._stream())
        assert kn.launches == {} and bool((out == SENTINEL).all()), (message, kn.launches)
    emb = md["input_embedder"]
    emb.train()
    try:
        with pytest.raises(RuntimeError, match="context_counts is eval-mode only"):
            emb(pts, context_counts=_cnt((200, 137, 64, k)))
    finally:
        emb.eval()


# ------------------------------------------------------------------------------------------------ callers
@contextlib.contextmanager
def _count_aware(embedder, on):
    embedder.count_aware = on           # (an instance attribute over the class default)
    try:
        yield
    finally:
        del embedder.count_aware


def test_inner_loop_embeds_a_ragged_batch_in_one_pass():
    cfg, md = _stack("c2_dgcnn_attn_spline")
    counts = (200, 137, 64, cfg["n_neighbors"])
    g = torch.Generator().manual_seed(11)
    e0, cnt = fa.pad_context_batch([torch.rand(c, 6, generator=g).to(DEV) for c in counts])
    e1 = torch.rand(4, 130, 6, generator=g).to(DEV)
    eps = [torch.randn(s, generator=g).to(DEV) for s in md["flow"].noise_shapes(4, 130)]
    emb = md["input_embedder"]
    with torch.no_grad():
        with _kernels() as kn:
            _, lp, _ = fa.inner_loop((e0, e1, None), md, cfg, eps=eps, context_counts=cnt)
        assert kn.count("gather_max") == 4 and kn.count("gather_max_counts_kernel") == 4, kn.launches
        with _count_aware(emb, False), _kernels() as kn_g:
            _, lp_g, _ = fa.inner_loop((e0, e1, None), md, cfg, eps=eps, context_counts=cnt)
        assert kn_g.count("gather_max") == 16 and kn_g.count("gather_max_counts_kernel") == 0, kn_g.launches
        # the rule of test 6, with the grouped path (every scene embedded alone here: four distinct counts) in the place of the scenes alone
        full = torch.rand(4, 200, 6, generator=g).to(DEV)
        _, lp_u, _ = fa.inner_loop((full, e1, None), md, cfg, eps=eps)
        uni_gap = max((lp_u[b:b + 1] - fa.inner_loop((full[b:b + 1], e1[b:b + 1], None), md, cfg, eps=[e[b:b + 1] for e in eps])[1]).abs().max().item() for b in range(4))
    _by_the_rule(uni_gap, (lp - lp_g).abs().max().item(), lambda: torch.equal(lp, lp_g), "inner_loop, count-aware against grouped")


@pytest.fixture(scope="module")
def scene():
    c0, c1 = SU.swapped_scene()
    return torch.from_numpy(c0).to(DEV), torch.from_numpy(c1).to(DEV), torch.from_numpy(U.centers_np()).to(DEV)


@pytest.fixture(scope="module")
def scene_model():
    """_model of tests/test_gpu_sparse_stage.py"""
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=2, sample_size=SU.N, n_samples_context=SU.M)
    cfg["final_voxel_size"], cfg["context_voxel_size"] = U.FINAL, U.CONTEXT
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    return cfg, md


def _same(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(-1.0), b.nan_to_num(-1.0))


@pytest.mark.parametrize("dense", [False, True], ids=["sampled", "dense"])
def test_scene_change_embeds_every_chunk_in_one_pass(scene, scene_model, dense, monkeypatch):
    c0, c1, centers = scene
    cfg, md = scene_model
    kw = dict(ground_height=U.GROUND, multiple=1.0, voxels_per_batch=7, min_context=256, **(dict(dense=True, block=256) if dense else {}))
    calls = []
    inner = model_initialization._embed_batch

    def counting(*a, **k):
        calls.append(1)
        return inner(*a, **k)
    monkeypatch.setattr(model_initialization, "_embed_batch", counting)
    torch.manual_seed(11)
    with _kernels() as kn:
        out, _ = fa.scene_change(c0, c1, md, cfg, centers, **kw)
    n_calls = len(calls)
    assert n_calls > 0 and kn.count("gather_max") == 4 * n_calls == kn.count("gather_max_counts_kernel"), (n_calls, kn.launches)
    del calls[:]
    torch.manual_seed(11)
    with _count_aware(md["input_embedder"], False), _kernels() as kn_g:
        out_g, _ = fa.scene_change(c0, c1, md, cfg, centers, **kw)
    assert len(calls) == n_calls and kn_g.count("gather_max") > 4 * n_calls and kn_g.count("gather_max_counts_kernel") == 0, kn_g.launches
    print(f"scene_change {'dense' if dense else 'sampled'}: {n_calls} _embed_batch calls; gather_max launches {kn.count('gather_max')} count-aware, "
          f"{kn_g.count('gather_max')} grouped")
    # the rule of test 6: is the uniform embedder batch-invariant at this shape (a chunk of 7 scenes of M = 1280 against its scenes alone)?
    handle = md["input_embedder"]._engine()
    pts = _clouds(7, SU.M, 6, 25)
    with torch.no_grad():
        uni = handle.embed(pts)
        uni_gap = max((uni[b:b + 1] - handle.embed(pts[b:b + 1])).abs().max().item() for b in range(7))
    assert torch.equal(out.isnan(), out_g.isnan())
    gap = (out.nan_to_num(-1.0) - out_g.nan_to_num(-1.0)).abs().max().item()
    print(f"  uniform embedder, 7 x {SU.M} against its scenes alone: max |d| {uni_gap:.2e}; change map count-aware against grouped: {gap:.2e}")
    # (the uniform gap is 0.0 on the MI355X, DESIGN 11i: the maps are then the same bytes.  A change score has no "scenes alone" side to
    # fall back on, so the same is asked where the gap is not 0 -- which is more than the rule of test 6 asks)
    assert _same(out, out_g)


def test_paconv_configuration_with_counts_keeps_the_grouping():
    """c3 (PAConv, two layers): inner_loop with counts goes through the equal-count grouping as before -- the embedder has no counted path"""
    cfg, md = _stack("c3_paconv_attn_affine", N=64)
    assert not getattr(md["input_embedder"], "count_aware", False)
    counts = (320, 256)
    g = torch.Generator().manual_seed(12)
    clouds = [torch.rand(c, 6, generator=g).to(DEV) for c in counts]
    e0, cnt = fa.pad_context_batch(clouds)
    e1 = torch.rand(2, 64, 6, generator=g).to(DEV)
    eps = [torch.randn(s, generator=g).to(DEV) for s in md["flow"].noise_shapes(2, 64)]
    with torch.no_grad():
        _, lp, _ = fa.inner_loop((e0, e1, None), md, cfg, eps=eps, context_counts=cnt)
        # what the parent computes: every group embedded by the embedder as it is, into zeros, then one flow call with the counts
        emb = torch.zeros(2, 320, cfg["input_embedding_dim"], device=DEV)
        for b, c in enumerate(counts):
            emb[b, :c] = md["input_embedder"](clouds[b][None])[0]
        ref = md["flow"].log_prob(e1, context=emb, extra_context=None, eps=eps, context_counts=cnt)
    assert bool(torch.isfinite(lp).all()) and torch.equal(lp, ref)
