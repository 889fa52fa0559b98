"""What the DGCNN embedder with per-scene point counts buys, on one GPU.  Host clock around a device synchronise,
3 warm-ups + 10 repeats, medians with min .. max; the baseline is this same build with `count_aware = False` on the embedder module
(the parent's Python path: one embedder call per distinct count), the two alternating in one process.  No gate: nothing here is asserted
in a test, except that both ways give the same bytes.

  * section 11g's case: C4, 115 flow layers, conditioned weights, 20 scenes, N = 1024, M = 1250, counts 256 .. 1250 evenly spread:
    inner_loop ragged count-aware, ragged grouped, and uniform;
  * section 11h's case: fa.scene_change on the swapped fixture scene (C4, 2 flow layers, voxels_per_batch = 16, min_context = 256), sampled
    and dense, both ways, with the embedder-call counts.

    python profiles/embed_counts_measure.py [--out profiles/embed_counts.json]
    rocprofv3 --kernel-trace --stats -d DIR -o knn -- python profiles/embed_counts_measure.py --trace      # per launch, a run of its own
    python profiles/embed_counts_measure.py --summarise DIR/<host>/<pid>_results.db [--out FILE]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

DEV = "cuda:0"
FINAL, CONTEXT = (3.0, 3.0, 4.0), (4.0, 4.0, 5.0)
KERNELS = ("knn_mfma_counts_kernel", "knn_mfma_kernel", "knn_counts_kernel", "knn_kernel", "gather_max_counts_kernel", "gather_max_kernel")


def timed(fn, warm=3, reps=10):
    import torch
    ts = []
    for _ in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = ts[warm:]
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": reps}, r


@contextlib.contextmanager
def count_aware(embedder, on):
    embedder.count_aware = on
    try:
        yield
    finally:
        del embedder.count_aware


def quiet_model(cfg, seed):
    import torch
    import flowcompare_amd as fa
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        return fa.initialize_flow(cfg, device=DEV, mode="test")


def ragged_inner_loop(res):
    """section 11g's case, built as bench.py builds its step (synth_pairs, condition_flow)"""
    import torch
    import flowcompare_amd as fa
    import bench
    from flowcompare_amd import engine
    from flowcompare_amd.conditioning import condition_flow
    B, N, M = 20, 1024, 1250
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", sample_size=N)
    md = quiet_model(cfg, 0)
    c0, c1, cx, cg = bench.synth_pairs(2, M, N, 999, DEV)
    condition_flow(md, cfg, (c0, c1, cx), eps=[torch.randn(2, N, cfg["latent_dim"] - cfg["input_dim"], generator=cg).to(DEV)])
    e0, e1, extra, g = bench.synth_pairs(B, M, N, 1000, DEV)
    eps = [torch.randn(s, generator=g).to(DEV) for s in md["flow"].noise_shapes(B, N)]
    counts = [round(256 + i * (M - 256) / (B - 1)) for i in range(B)]
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    emb = md["input_embedder"]
    before = engine.lib().fc_debug_fp16_fallbacks()
    with torch.no_grad():
        def ragged():
            return fa.inner_loop((e0, e1, extra), md, cfg, eps=eps, context_counts=cnt)[1]
        # alternating: aware, grouped, uniform, three rounds; the medians over each way's 30 repeats
        rounds = {"inner_loop_ragged_count_aware": [], "inner_loop_ragged_grouped": [], "inner_loop_uniform": []}
        for _ in range(3):
            t, lp_a = timed(ragged)
            rounds["inner_loop_ragged_count_aware"].append(t)
            with count_aware(emb, False):
                t, lp_g = timed(ragged)
            rounds["inner_loop_ragged_grouped"].append(t)
            t, _ = timed(lambda: fa.inner_loop((e0, e1, extra), md, cfg, eps=eps)[1])
            rounds["inner_loop_uniform"].append(t)
        # the embedder alone, both ways
        x0 = e0[:, :, :cfg["input_dim"]].contiguous()
        t_emb_a, ea = timed(lambda: emb(x0, context_counts=cnt, count_range=(min(counts), max(counts))))
        t_emb_u, _ = timed(lambda: emb(x0))
        def grouped_embed():
            return [emb(x0[b:b + 1, :c].contiguous()) for b, c in enumerate(counts)]
        t_emb_g, eg = timed(grouped_embed)
    out = {"shape": {"B": B, "N": N, "M": M, "counts": counts, "config": "c4_dgcnn_attn_extra_affine", "layers": cfg["n_flow_layers"]}}
    for k, v in rounds.items():
        out[k] = {"median_ms": round(statistics.median(r["median_ms"] for r in v), 3), "min_ms": min(r["min_ms"] for r in v),
                  "max_ms": max(r["max_ms"] for r in v), "rounds_median_ms": [r["median_ms"] for r in v], "reps": "3 rounds x 10"}
    out["embedder_counted_one_call"], out["embedder_uniform_one_call"], out["embedder_one_call_per_count"] = t_emb_a, t_emb_u, t_emb_g
    out["log_probs_equal_bitwise"] = bool(torch.equal(lp_a, lp_g))
    out["embeddings_equal_bitwise"] = all(bool(torch.equal(ea[b:b + 1, :c], eg[b])) and bool((ea[b, c:] == 0).all()) for b, c in enumerate(counts))
    out["fp16_fallbacks"] = engine.lib().fc_debug_fp16_fallbacks() - before
    res["ragged_inner_loop"] = out
    print("ragged_inner_loop", json.dumps(out), flush=True)


def scene_change(res):
    """section 11h's case"""
    import torch
    import flowcompare_amd as fa
    import sparse_stage_util as SU
    import scene_stage_util as U
    f0, f1 = (torch.from_numpy(c).to(DEV) for c in SU.swapped_scene())
    fc = torch.from_numpy(U.centers_np()).to(DEV)
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=2, sample_size=SU.N, n_samples_context=SU.M)
    cfg["final_voxel_size"], cfg["context_voxel_size"] = FINAL, CONTEXT
    md = quiet_model(cfg, 0)
    emb = md["input_embedder"]
    calls = [0]
    emb.register_forward_hook(lambda *a: calls.__setitem__(0, calls[0] + 1))
    out = {"config": "c4_dgcnn_attn_extra_affine, 2 flow layers", "voxels_per_batch": 16, "min_context": 256}
    for dense in (False, True):
        def run():
            torch.manual_seed(11)
            calls[0] = 0
            return fa.scene_change(f0, f1, md, cfg, fc, ground_height=0.25, voxels_per_batch=16, dense=dense, min_context=256)
        rounds = {"count_aware": [], "grouped": []}
        for _ in range(3):
            t, (map_a, st) = timed(run, warm=2, reps=5)
            rounds["count_aware"].append(dict(t, embedder_calls=calls[0]))
            with count_aware(emb, False):
                t, (map_g, _) = timed(run, warm=2, reps=5)
            rounds["grouped"].append(dict(t, embedder_calls=calls[0]))
        key = "dense" if dense else "sampled"
        out[key] = {w: {"median_ms": round(statistics.median(r["median_ms"] for r in v), 3), "min_ms": min(r["min_ms"] for r in v),
                        "max_ms": max(r["max_ms"] for r in v), "embedder_calls": v[0]["embedder_calls"], "reps": "3 rounds x 5"} for w, v in rounds.items()}
        out[key]["voxels"] = st.voxel.numel()
        out[key]["points_scored"] = int(torch.isfinite(map_a).sum())
        out[key]["maps_equal_bitwise"] = bool(torch.equal(map_a.isnan(), map_g.isnan()) and torch.equal(map_a.nan_to_num(-1.0), map_g.nan_to_num(-1.0)))
    res["scene_change_fixture"] = out
    print("scene_change_fixture", json.dumps(out), flush=True)


def measure(out_path):
    res = {"how": "host clock around work that ends in a device synchronise; warm-ups then repeats; count-aware and grouped (count_aware = False on "
                  "the embedder module: one embedder call per distinct count, the parent's Python path) alternate in one process on one library"}
    ragged_inner_loop(res)
    scene_change(res)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def trace():
    """the k-NN kernels alone, for rocprofv3 --kernel-trace: 16 x 4096 at the embedder's four feature widths, uniform, counted with full counts
    and counted with counts spread evenly over 1024 .. 4096 (both kernels: the scenes below 2048 take the lane kernel); 5 launches each.
    Under FCFLOW_LIB (a library without the counted entry) the uniform launches only."""
    import torch
    from flowcompare_amd import engine
    B, M, k = 16, 4096, 40
    has_counts = hasattr(engine.lib(), "fc_op_knn_counts_f32")
    full = torch.full((B,), M, dtype=torch.int32, device=DEV)
    spread = torch.tensor([round(1024 + i * (M - 1024) / (B - 1)) for i in range(B)], dtype=torch.int32, device=DEV)
    for C in (6, 64, 128):
        f = (torch.rand(B, M, C, generator=torch.Generator().manual_seed(71)) * 2 - 1).to(DEV)
        g = f[:, :1024].contiguous()                       # the lane kernel at 16 x 1024, uniform and full counts
        for x, cs in ((f, (None, full, spread)), (g, (None, torch.full((B,), 1024, dtype=torch.int32, device=DEV)))):
            for c in cs if has_counts else (None,):
                for _ in range(5):
                    engine.op_knn(x, k, counts=c)
    torch.cuda.synchronize()


def summarise(path, out_path):
    """rocprofv3's kernel trace (the `kernels` view of its results .db) -> per-launch microseconds of the k-NN kernels, grouped by kernel and
    grid; launches of one group come in the order of trace(): uniform; full counts; spread counts"""
    import sqlite3
    rows = sqlite3.connect(path).execute("select name, grid_x, grid_y, workgroup_x, end - start from kernels order by start").fetchall()
    groups = {}
    for name, gx, gy, wg, ns in rows:
        short = next((k for k in KERNELS if f"fc::{k}<" in name or f"fc::{k}(" in name or name in (k, f"fc::{k}")), None)
        if short is not None:
            groups.setdefault((name.split("(")[0].replace("void ", ""), gx // max(wg, 1), gy), []).append(ns / 1e3)
    res = [{"kernel": k, "grid": [gx, gy], "launches": len(v), "us_median": round(statistics.median(v), 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
            "us_by_fives": [round(statistics.median(v[i:i + 5]), 1) for i in range(0, len(v), 5)]} for (k, gx, gy), v in sorted(groups.items())]
    print(json.dumps(res, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/embed_counts.json; with --summarise: print only")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", metavar="RESULTS_DB")
    a = ap.parse_args()
    if a.summarise is not None:
        summarise(a.summarise, a.out)
    elif a.trace:
        trace()
    else:
        measure(a.out or os.path.join(ROOT, "profiles", "embed_counts.json"))
