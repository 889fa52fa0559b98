"""The PAConv embedder with per-scene point counts (include/fcflow_paconv_counts.h) on the GPU.  Every comparison
has an existing entry on its other side: the uniform call on the scene alone, as xyz[b:b+1, :c] / pts[b:b+1, :c].

operators  engine.op_fps_counts against engine.op_fps, engine.op_paconv_knn_counts against fc_op_paconv_knn_f32, on random clouds and on
           lattices with exact ties (the literal heap path of the 32-NN, the bit-reversed tie rule of the sampling): integer results, always
           torch.equal;
engine     PaconvHandle.embed_counts against PaconvHandle.embed by the rule of tests/test_gpu_embed_counts.py (restated below), pad rows
           of pts and of the output, the LDS / global boundary of the sampling, refusals;
callers    inner_loop and scene_change with `count_aware = True` embed a ragged batch in ONE PAConv call, with the results of the grouping."""
import contextlib
import functools
import io

import pytest
import torch

import flowcompare_amd as fa
import scene_stage_util as U
import sparse_stage_util as SU
from flowcompare_amd import engine, model_initialization

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77
COUNTS = (1100, 1024, 1023, 512, 256)        # n = M = 1100: per-scene virtual thread counts 1024 / 1024 / 512 / 512 / 256
SMALL = (68, 64, 63, 32, 16)                 # the level-2 sizes of COUNTS (n = 68): n_b < k, n_b == k and the index-0 tail of the 32-NN


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


def _by_the_rule(uni_gap, gap, equal, what):
    """bit for bit where the uniform path is batch-invariant on this input, otherwise no further from the scenes alone than the uniform batch is"""
    print(f"{what}: uniform batch against its scenes alone max |d| {uni_gap:.2e}; counted batch against its scenes alone {gap:.2e}")
    if uni_gap == 0.0:
        assert equal(), what
    else:
        assert gap <= uni_gap, what


def _opt_n_threads(n):
    """opt_n_threads of the sampling kernel: the largest power of two <= n, at most 1024"""
    return min(1024, 1 << (n.bit_length() - 1))


# ------------------------------------------------------------------------------------------------ operators
@functools.lru_cache(maxsize=None)
def _op_clouds():
    """[5, 1100, 3] clouds: random points; an integer lattice (the 8 x 8 x 8 grid of _pointops_clouds in tests/test_gpu_ops.py, tiled along x to
    1100 rows: exact distance ties everywhere); the non-cubic lattice tiled in place (ties at distance 0 as well).  Every scene holds the
    lattice's rows in its own order, so that its first count_b rows are its own subset."""
    g = torch.Generator().manual_seed(31)
    lat = torch.stack(torch.meshgrid(torch.arange(8.), torch.arange(8.), torch.arange(8.), indexing="ij"), -1).reshape(-1, 3)
    i = torch.arange(1100)
    tiled = lat[i % 512] + torch.tensor([8.0, 0.0, 0.0]) * (i // 512)[:, None]
    dup = lat[i % 512] * torch.tensor([1.0, 0.5, 0.25])
    order = [torch.randperm(1100, generator=g) for _ in range(5)]
    return {"random": torch.rand(5, 1100, 3, generator=g).to(DEV), "lattice": torch.stack([tiled[o] for o in order]).to(DEV),
            "lattice+duplicates": torch.stack([dup[o] for o in order]).to(DEV)}


def _pitch4(x):
    return torch.cat([x, torch.zeros_like(x[..., :1])], -1).contiguous()


def _knn_alone(x4, q4, k):
    """fc_op_paconv_knn_f32 on one scene: x4 [1, n, 4], q4 [1, m, 4] -> [1, m, k]"""
    n, m = x4.shape[1], q4.shape[1]
    out = torch.full((1, m, k), -1, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        engine.lib().fc_op_paconv_knn_f32(engine._ptr(x4), engine._ptr(q4), engine._ptr(out), 1, n, m, k, engine._stream())
    return out


@pytest.mark.parametrize("cloud", ["random", "lattice", "lattice+duplicates"])
def test_fps_with_counts_equals_every_scene_alone(cloud):
    assert [_opt_n_threads(c) for c in COUNTS] == [1024, 1024, 512, 512, 256]
    xyz = _op_clouds()[cloud]
    with _kernels() as kn:
        got = engine.op_fps_counts(xyz, _cnt(COUNTS))
    assert kn.count("fc::fps_kernel") == 1, kn.launches
    assert tuple(got.shape) == (5, 275)
    for b, c in enumerate(COUNTS):
        alone = engine.op_fps(xyz[b:b + 1, :c].contiguous(), c >> 2)
        assert torch.equal(got[b:b + 1, :c >> 2], alone), f"{cloud}: scene {b} ({c} points) differs from its sampling alone"
        assert bool((got[b, c >> 2:] == -1).all()), f"{cloud}: scene {b}: picks >= {c >> 2} are not -1"
    assert torch.equal(engine.op_fps_counts(xyz, _cnt([1100] * 5)), engine.op_fps(xyz, 275)), "full counts: the bytes of the uniform call"


def _knn_case(xyz, counts, k=32):
    """queries = every scene's own FPS picks (m_b = n_b >> 2); -> (x4 [B, n, 4], q4 [B, m, 4] with zeros behind the scene's queries, counts_m)"""
    B, n, _ = xyz.shape
    m = n >> 2
    q = torch.zeros(B, m, 3, device=DEV)
    for b, c in enumerate(counts):
        picks = engine.op_fps(xyz[b:b + 1, :c].contiguous(), c >> 2)[0].long()
        q[b, :c >> 2] = xyz[b, picks]
    return _pitch4(xyz), _pitch4(q), tuple(c >> 2 for c in counts)


def _check_knn(xyz, counts, what, k=32):
    x4, q4, counts_m = _knn_case(xyz, counts, k)
    with _kernels() as kn:
        got = engine.op_paconv_knn_counts(x4, q4, _cnt(counts), _cnt(counts_m), k)
    assert kn.count("fc::knn_xyz_kernel") == 1, kn.launches
    for b, (c, mb) in enumerate(zip(counts, counts_m)):
        alone = _knn_alone(x4[b:b + 1, :c].contiguous(), q4[b:b + 1, :mb].contiguous(), k)
        assert torch.equal(got[b:b + 1, :mb], alone), f"{what}: scene {b} ({c} points, {mb} queries) differs from its search alone"
        assert bool((got[b, mb:] == 0).all()), f"{what}: scene {b}: rows >= {mb} are not zeros"
        if c < k:
            assert bool((got[b, :mb, c:] == 0).all()), f"{what}: scene {b}: the tail behind {c} neighbours is not index 0"
    return got


@pytest.mark.parametrize("cloud", ["random", "lattice", "lattice+duplicates"])
def test_knn_with_counts_equals_every_scene_alone(cloud):
    """n_b = 1100 (alone: 32 list entries per lane), 512 (alone: 8) and 256 in one launch; on the lattices neighbouring distances tie, so
    lane 0 re-runs the query through the reference's heap over the scene's own n_b rows"""
    xyz = _op_clouds()[cloud]
    if cloud != "random":                                      # the tie the heap path needs is there: query 0 of every scene
        for b, c in enumerate(COUNTS):
            d = ((xyz[b, :c] - xyz[b, 0]) ** 2).sum(-1).sort().values[:33]
            assert bool((d[1:] == d[:-1]).any())
    _check_knn(xyz, COUNTS, cloud)
    full = _check_knn(xyz, (1100,) * 5, f"{cloud}, full counts")
    x4, q4, _ = _knn_case(xyz, (1100,) * 5)
    out = torch.empty_like(full)
    with torch.cuda.device(DEV):
        engine.lib().fc_op_paconv_knn_f32(engine._ptr(x4), engine._ptr(q4), engine._ptr(out), 5, 1100, 275, 32, engine._stream())
    assert torch.equal(full, out), "full counts: the bytes of the uniform call"


@pytest.mark.parametrize("cloud", ["random", "lattice", "lattice+duplicates"])
def test_knn_with_counts_below_k(cloud):
    """the level-2 sizes: n = 68 with n_b = 68 / 64 / 63 / 32 / 16 against k = 32"""
    _check_knn(_op_clouds()[cloud][:, :68].contiguous(), SMALL, f"{cloud}, n = 68")


# ------------------------------------------------------------------------------------------------ engine
@functools.lru_cache(maxsize=None)
def _stack(name, N=64, **kw):
    """Two layers of a named configuration, built like _stack of tests/test_gpu_embed_counts.py"""
    cfg = fa.named_config(name, n_flow_layers=2, sample_size=N, **kw)
    torch.manual_seed(7)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    return cfg, md


def _clouds(B, M, C, seed):
    return torch.rand(B, M, C, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _gaps(handle, pts, counts):
    """(uniform gap, counted gap, counted result, scenes alone, uniform result): the B-scene uniform call against its B = 1 calls through the
    existing entry, and the counted call against the scenes alone on their own rows"""
    B = pts.shape[0]
    uniform = handle.embed(pts)
    uni_gap = max((uniform[b:b + 1] - handle.embed(pts[b:b + 1])).abs().max().item() for b in range(B))
    got = handle.embed_counts(pts, _cnt(counts))
    alone = [handle.embed(pts[b:b + 1, :c].contiguous()) for b, c in enumerate(counts)]
    gap = max((got[b:b + 1, :c] - alone[b]).abs().max().item() for b, c in enumerate(counts))
    return uni_gap, gap, got, alone, uniform


@functools.lru_cache(maxsize=None)
def _engine_case():
    cfg, md = _stack("c3_paconv_attn_affine")
    handle = md["input_embedder"]._engine()
    pts = _clouds(5, 1100, cfg["input_dim"], 21)
    with torch.no_grad():
        return (handle, pts) + _gaps(handle, pts, COUNTS)


def test_handle_with_counts_equals_every_scene_alone():
    # the smallest shapes with 1, 2 and 3 known points in the last propagation level and n < k at levels 2 and 3
    assert [[c >> 2 * l for l in range(1, 5)] for c in COUNTS] == [[275, 68, 17, 4], [256, 64, 16, 4], [255, 63, 15, 3], [128, 32, 8, 2], [64, 16, 4, 1]]
    handle, pts, uni_gap, gap, got, alone, uniform = _engine_case()
    _by_the_rule(uni_gap, gap, lambda: all(torch.equal(got[b:b + 1, :c], alone[b]) for b, c in enumerate(COUNTS)), "PAConv embed, M = 1100")
    with torch.no_grad():
        # output rows >= c are exactly 0, from a buffer the test prefilled with NaN
        out = torch.full_like(got, float("nan"))
        assert handle.embed_counts(pts, _cnt(COUNTS), out=out) is out and torch.equal(out, got)
        for b, c in enumerate(COUNTS):
            assert bool((got[b, c:] == 0).all()) and bool(torch.isfinite(got[b]).all())
        assert torch.equal(handle.embed_counts(pts, _cnt([1100] * 5)), uniform), "full counts: the bytes of the uniform call"
        # count_range from a caller that has read the counts back: the same bytes
        assert torch.equal(handle.embed_counts(pts, _cnt(COUNTS), count_range=(min(COUNTS), max(COUNTS))), got)
        # one call: four sampling launches, not four per scene
        with _kernels() as kn:
            handle.embed_counts(pts, _cnt(COUNTS))
        assert kn.count("fc::fps_kernel") == 4, kn.launches


def test_pad_rows_of_the_points_do_not_matter():
    handle, pts, _, _, got, _, _ = _engine_case()
    cnt = _cnt(COUNTS)
    pad = torch.arange(1100, device=DEV)[None, :, None] >= cnt[:, None, None]
    lib = engine.lib()
    with torch.no_grad():
        zeros = handle.embed_counts(pts.masked_fill(pad, 0.0), cnt)
        assert torch.equal(got, zeros)
        before = lib.fc_debug_fp16_fallbacks()
        for fill in (float("nan"), 1e30):
            filled = handle.embed_counts(pts.masked_fill(pad, fill), cnt)
            assert bool(torch.isfinite(filled).all()) and torch.equal(filled, zeros), fill
        assert lib.fc_debug_fp16_fallbacks() == before


def test_a_batch_across_the_lds_boundary_of_the_sampling():
    """M = 8200: above 8192 points per scene the sampling reads coordinates and running distances from memory.  Scene 1 (8192 points) runs
    the LDS kernel alone and the memory kernel in the batch; the picks are the same, and so is the embedding, by the rule."""
    counts = (8200, 8192, 256)
    cfg, md = _stack("c3_paconv_attn_affine")
    handle = md["input_embedder"]._engine()
    pts = _clouds(3, 8200, cfg["input_dim"], 23)
    xyz = pts[:, :, :3].contiguous()
    picks = engine.op_fps_counts(xyz, _cnt(counts))
    for b, c in enumerate(counts):
        assert torch.equal(picks[b:b + 1, :c >> 2], engine.op_fps(xyz[b:b + 1, :c].contiguous(), c >> 2)), f"scene {b} ({c} points)"
        assert bool((picks[b, c >> 2:] == -1).all())
    with torch.no_grad():
        uni_gap, gap, got, alone, _ = _gaps(handle, pts, counts)
    _by_the_rule(uni_gap, gap, lambda: all(torch.equal(got[b:b + 1, :c], alone[b]) for b, c in enumerate(counts)), "PAConv embed, M = 8200")
    for b, c in enumerate(counts):
        assert bool((got[b, c:] == 0).all()) and bool(torch.isfinite(got[b]).all())


@pytest.mark.parametrize("lo,hi,null,message", [
    (255, 320, False, "PAConv embedder needs at least 256 context points"), (256, 321, False, "256 <= count_min <= count_max <= M"),
    (300, 256, False, "256 <= count_min <= count_max <= M"), (256, 320, True, "null counts"),
])
def test_refusals_return_their_status_and_launch_nothing(lo, hi, null, message):
    cfg, md = _stack("c3_paconv_attn_affine")
    handle = md["input_embedder"]._engine()
    pts = _clouds(2, 320, cfg["input_dim"], 24)
    cnt = _cnt((320, 256))
    out = torch.full((2, 320, handle.out_dim), float(SENTINEL), device=DEV)
    ws = torch.empty(1 << 27, dtype=torch.uint8, device=DEV)
    with _kernels() as kn:
        with pytest.raises(engine.FcError, match=message) as e:
            engine.lib().fc_paconv_embed_counts_f32(handle._h, engine._ptr(pts), None if null else engine._ptr(cnt), lo, hi, engine._ptr(out), 2, 320,
                                                    engine._ptr(ws), ws.numel(), engine._stream())
    assert e.value.code == 1
    assert kn.launches == {} and bool((out == SENTINEL).all()), (message, kn.launches)


def test_binding_and_operators_refuse_by_message():
    cfg, md = _stack("c3_paconv_attn_affine")
    handle = md["input_embedder"]._engine()
    pts = _clouds(2, 320, cfg["input_dim"], 24)
    with pytest.raises(RuntimeError, match="count 255 is below 256"):
        handle.embed_counts(pts, _cnt((320, 255)))
    with pytest.raises(RuntimeError, match=r"counts out of range: count 321 is not in \[1, 320\]"):
        handle.embed_counts(pts, _cnt((321, 256)))
    with pytest.raises(RuntimeError, match=r"counts must have shape \[B\] with B = 2"):
        handle.embed_counts(pts, _cnt((320, 256, 256)))
    with pytest.raises(RuntimeError, match="PaconvHandle.embed: this embedder has no path with per-scene point counts"):
        handle.embed(pts, counts=_cnt((320, 256)))
    xyz = pts[:, :, :3].contiguous()
    idx = torch.full((2, 80), SENTINEL, dtype=torch.int32, device=DEV)
    L = engine.lib()
    for args, message in (((engine._ptr(xyz), engine._ptr(_cnt((320, 256))), 3, 320, engine._ptr(idx), 2, 320, 80), "4 <= count_min <= count_max <= n"),
                          ((engine._ptr(xyz), engine._ptr(_cnt((320, 256))), 256, 321, engine._ptr(idx), 2, 320, 80), "4 <= count_min <= count_max <= n"),
                          ((engine._ptr(xyz), engine._ptr(_cnt((320, 256))), 256, 320, engine._ptr(idx), 2, 320, 79), "m must be n >> 2"),
                          ((engine._ptr(xyz), None, 256, 320, engine._ptr(idx), 2, 320, 80), "null pointer")):
        with _kernels() as kn:
            with pytest.raises(engine.FcError, match=message) as e:
                L.fc_op_fps_counts_f32(*args, engine._stream())
        assert e.value.code == 1 and kn.launches == {} and bool((idx == SENTINEL).all()), (message, kn.launches)
    emb = md["input_embedder"]
    emb.train()
    try:
        with pytest.raises(RuntimeError, match="context_counts is eval-mode only"):
            emb(pts, context_counts=_cnt((320, 256)))
    finally:
        emb.eval()


# ------------------------------------------------------------------------------------------------ callers
@contextlib.contextmanager
def _count_aware(embedder, on):
    embedder.count_aware = on           # (an instance attribute: the class has none, which _embed_batch reads as False)
    try:
        yield
    finally:
        del embedder.count_aware


def test_inner_loop_embeds_a_ragged_batch_in_one_call():
    cfg, md = _stack("c3_paconv_attn_affine")
    emb = md["input_embedder"]
    assert not getattr(emb, "count_aware", False)
    counts = (320, 256)
    g = torch.Generator().manual_seed(12)
    e0, cnt = fa.pad_context_batch([torch.rand(c, 6, generator=g).to(DEV) for c in counts])
    e1 = torch.rand(2, 64, 6, generator=g).to(DEV)
    eps = [torch.randn(s, generator=g).to(DEV) for s in md["flow"].noise_shapes(2, 64)]
    with torch.no_grad():
        with _count_aware(emb, True), _kernels() as kn:
            _, lp, _ = fa.inner_loop((e0, e1, None), md, cfg, eps=eps, context_counts=cnt)
        assert kn.count("fc::fps_kernel") == 4, kn.launches                 # one PAConv call: one sampling launch per level
        with _kernels() as kn_g:
            _, lp_g, _ = fa.inner_loop((e0, e1, None), md, cfg, eps=eps, context_counts=cnt)
        assert kn_g.count("fc::fps_kernel") == 8, kn_g.launches             # the grouping: one call per distinct count
        full = torch.rand(2, 320, 6, generator=g).to(DEV)
        _, lp_u, _ = fa.inner_loop((full, e1, None), md, cfg, eps=eps)
        uni_gap = max((lp_u[b:b + 1] - fa.inner_loop((full[b:b + 1], e1[b:b + 1], None), md, cfg, eps=[e[b:b + 1] for e in eps])[1]).abs().max().item() for b in range(2))
    assert bool(torch.isfinite(lp).all())
    _by_the_rule(uni_gap, (lp - lp_g).abs().max().item(), lambda: torch.equal(lp, lp_g), "inner_loop, count-aware against grouped")
    emb.train()
    try:
        with _count_aware(emb, True), pytest.raises(RuntimeError, match="context_counts is eval-mode only"):
            fa.inner_loop((e0, e1, None), md, cfg, eps=eps, context_counts=cnt)
    finally:
        emb.eval()


@pytest.fixture(scope="module")
def scene():
    """the fixture scene of tests/scene_stage_util.py with the roles swapped (tests/sparse_stage_util.py), so that context boxes are ragged"""
    c0, c1 = SU.swapped_scene()
    return torch.from_numpy(c0).to(DEV), torch.from_numpy(c1).to(DEV), torch.from_numpy(U.centers_np()).to(DEV)


@pytest.fixture(scope="module")
def scene_model():
    cfg = fa.named_config("c3_paconv_attn_affine", n_flow_layers=2, sample_size=SU.N, n_samples_context=SU.M)
    cfg["final_voxel_size"], cfg["context_voxel_size"] = U.FINAL, U.CONTEXT
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    return cfg, md


def _same(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(-1.0), b.nan_to_num(-1.0))


@pytest.mark.parametrize("dense", [False, True], ids=["sampled", "dense"])
def test_scene_change_embeds_every_chunk_in_one_call(scene, scene_model, dense, monkeypatch):
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
    with _count_aware(md["input_embedder"], True), _kernels() as kn:
        out, _ = fa.scene_change(c0, c1, md, cfg, centers, **kw)
    n_calls = len(calls)
    assert n_calls > 0 and kn.count("fc::fps_kernel") == 4 * n_calls, (n_calls, kn.launches)       # one embedder call per chunk and pass
    del calls[:]
    torch.manual_seed(11)
    with _kernels() as kn_g:
        out_g, _ = fa.scene_change(c0, c1, md, cfg, centers, **kw)
    assert len(calls) == n_calls and kn_g.count("fc::fps_kernel") > 4 * n_calls, kn_g.launches
    print(f"scene_change {'dense' if dense else 'sampled'}: {n_calls} _embed_batch calls; PAConv calls {kn.count('fc::fps_kernel') // 4} count-aware, "
          f"{kn_g.count('fc::fps_kernel') // 4} grouped")
    assert bool(out.isfinite().any())
    gap = (out.nan_to_num(-1.0) - out_g.nan_to_num(-1.0)).abs().max().item()
    print(f"  change map count-aware against grouped: max |d| {gap:.2e}")
    assert _same(out, out_g)
