"""What the PAConv embedder with per-scene point counts buys, on one GPU.  Host clock around a device synchronise,
warm-ups then repeats, medians with min .. max; the baseline is this same build with `count_aware` unset on the embedder module (the
grouping: one embedder call per distinct count), the two alternating in one process, three rounds.  No gate: nothing here is asserted in a
test; whether both ways give the same bytes is recorded.

  * section 11i's inner_loop case on C3: 20 scenes, N = 1024, M = 1250, counts 256 .. 1250 evenly spread: inner_loop ragged count-aware,
    ragged grouped, and uniform; the embedder alone counted, uniform and one call per count;
  * fa.scene_change on the swapped fixture scene (C3, 2 flow layers, voxels_per_batch = 16, min_context = 256), sampled and dense, both
    ways, with the embedder-call counts.

    python profiles/paconv_counts_measure.py [--out profiles/paconv_counts.json]
    python profiles/paconv_counts_measure.py --ab-parent PARENT_LIB [--out profiles/paconv_counts_ab_parent.json]
        # the uniform path against the parent commit's library: `bench.py --config c3_paconv_attn_affine` alternating, three pairs
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

DEV = "cuda:0"
FINAL, CONTEXT = (3.0, 3.0, 4.0), (4.0, 4.0, 5.0)
C3 = "c3_paconv_attn_affine"


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
    if on:
        embedder.count_aware = True
    try:
        yield
    finally:
        if on:
            del embedder.count_aware


def quiet_model(cfg, seed):
    import torch
    import flowcompare_amd as fa
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        return fa.initialize_flow(cfg, device=DEV, mode="test")


def over_rounds(v):
    return {"median_ms": round(statistics.median(r["median_ms"] for r in v), 3), "min_ms": min(r["min_ms"] for r in v),
            "max_ms": max(r["max_ms"] for r in v), "rounds_median_ms": [r["median_ms"] for r in v]}


def ragged_inner_loop(res):
    """section 11i's case on C3, built as bench.py builds its step (synth_pairs, condition_flow)"""
    import torch
    import flowcompare_amd as fa
    import bench
    from flowcompare_amd import engine
    from flowcompare_amd.conditioning import condition_flow
    B, N, M = 20, 1024, 1250
    cfg = fa.named_config(C3, sample_size=N)
    md = quiet_model(cfg, 0)
    c0, c1, cx, cg = bench.synth_pairs(2, M, N, 999, DEV)
    if not cfg.get("using_extra_context"):
        cx = None
    condition_flow(md, cfg, (c0, c1, cx), eps=[torch.randn(2, N, cfg["latent_dim"] - cfg["input_dim"], generator=cg).to(DEV)])
    e0, e1, extra, g = bench.synth_pairs(B, M, N, 1000, DEV)
    if not cfg.get("using_extra_context"):
        extra = None
    eps = [torch.randn(s, generator=g).to(DEV) for s in md["flow"].noise_shapes(B, N)]
    counts = [round(256 + i * (M - 256) / (B - 1)) for i in range(B)]
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    emb = md["input_embedder"]
    before = engine.lib().fc_debug_fp16_fallbacks()
    with torch.no_grad():
        def ragged():
            return fa.inner_loop((e0, e1, extra), md, cfg, eps=eps, context_counts=cnt)[1]
        rounds = {"inner_loop_ragged_count_aware": [], "inner_loop_ragged_grouped": [], "inner_loop_uniform": []}
        x0 = e0[:, :, :cfg["input_dim"]].contiguous()
        emb_rounds = {"embedder_counted_one_call": [], "embedder_uniform_one_call": [], "embedder_one_call_per_count": []}

        def grouped_embed():
            return [emb(x0[b:b + 1, :c].contiguous()) for b, c in enumerate(counts)]
        for _ in range(3):
            with count_aware(emb, True):
                t, lp_a = timed(ragged)
            rounds["inner_loop_ragged_count_aware"].append(t)
            t, lp_g = timed(ragged)
            rounds["inner_loop_ragged_grouped"].append(t)
            t, _ = timed(lambda: fa.inner_loop((e0, e1, extra), md, cfg, eps=eps)[1])
            rounds["inner_loop_uniform"].append(t)
            t, ea = timed(lambda: emb(x0, context_counts=cnt, count_range=(min(counts), max(counts))))
            emb_rounds["embedder_counted_one_call"].append(t)
            t, _ = timed(lambda: emb(x0))
            emb_rounds["embedder_uniform_one_call"].append(t)
            t, eg = timed(grouped_embed)
            emb_rounds["embedder_one_call_per_count"].append(t)
    out = {"shape": {"B": B, "N": N, "M": M, "counts": counts, "config": C3, "layers": cfg["n_flow_layers"]}, "reps": "3 rounds x 10"}
    for k, v in list(rounds.items()) + list(emb_rounds.items()):
        out[k] = over_rounds(v)
    out["log_probs_equal_bitwise"] = bool(torch.equal(lp_a, lp_g))
    out["log_probs_max_abs_diff"] = float((lp_a - lp_g).abs().max())
    out["embeddings_equal_bitwise"] = all(bool(torch.equal(ea[b:b + 1, :c], eg[b])) and bool((ea[b, c:] == 0).all()) for b, c in enumerate(counts))
    out["fp16_fallbacks"] = engine.lib().fc_debug_fp16_fallbacks() - before
    res["ragged_inner_loop"] = out
    print("ragged_inner_loop", json.dumps(out), flush=True)


def scene_change(res):
    import torch
    import flowcompare_amd as fa
    import sparse_stage_util as SU
    import scene_stage_util as U
    f0, f1 = (torch.from_numpy(c).to(DEV) for c in SU.swapped_scene())
    fc = torch.from_numpy(U.centers_np()).to(DEV)
    cfg = fa.named_config(C3, n_flow_layers=2, sample_size=SU.N, n_samples_context=SU.M)
    cfg["final_voxel_size"], cfg["context_voxel_size"] = FINAL, CONTEXT
    md = quiet_model(cfg, 0)
    emb = md["input_embedder"]
    calls = [0]
    emb.register_forward_hook(lambda *a: calls.__setitem__(0, calls[0] + 1))
    out = {"config": C3 + ", 2 flow layers", "voxels_per_batch": 16, "min_context": 256, "reps": "3 rounds x 5"}
    for dense in (False, True):
        def run():
            torch.manual_seed(11)
            calls[0] = 0
            return fa.scene_change(f0, f1, md, cfg, fc, ground_height=0.25, voxels_per_batch=16, dense=dense, min_context=256)
        rounds = {"count_aware": [], "grouped": []}
        for _ in range(3):
            with count_aware(emb, True):
                t, (map_a, st) = timed(run, warm=2, reps=5)
            rounds["count_aware"].append(dict(t, embedder_calls=calls[0]))
            t, (map_g, _) = timed(run, warm=2, reps=5)
            rounds["grouped"].append(dict(t, embedder_calls=calls[0]))
        key = "dense" if dense else "sampled"
        out[key] = {w: dict(over_rounds(v), embedder_calls=v[0]["embedder_calls"]) for w, v in rounds.items()}
        out[key]["voxels"] = st.voxel.numel()
        out[key]["points_scored"] = int(torch.isfinite(map_a).sum())
        out[key]["maps_equal_bitwise"] = bool(torch.equal(map_a.isnan(), map_g.isnan()) and torch.equal(map_a.nan_to_num(-1.0), map_g.nan_to_num(-1.0)))
    res["scene_change_fixture"] = out
    print("scene_change_fixture", json.dumps(out), flush=True)


def measure(out_path):
    res = {"how": "host clock around work that ends in a device synchronise; warm-ups then repeats; count-aware (count_aware = True on the embedder "
                  "module) and grouped (the attribute unset: one embedder call per distinct count) alternate in one process on one library"}
    ragged_inner_loop(res)
    scene_change(res)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def ab_parent(parent_lib, out_path, pairs=3):
    """bench.py on C3 with the parent commit's library (FCFLOW_LIB) and this build alternating, every run a process of its own"""
    import numpy as np
    runs, same = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(1, pairs + 1):
            for who in ("parent", "new"):
                d = os.path.join(tmp, f"{who}{i}")
                env = dict(os.environ)
                env.pop("FCFLOW_LIB", None)
                if who == "parent":
                    env["FCFLOW_LIB"] = os.path.abspath(parent_lib)
                r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", C3, "--steps", "20", "--warmup", "5",
                                    "--dump-outputs", d], env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    raise SystemExit(f"bench.py failed in run {who}{i} (exit {r.returncode})")
                line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                runs.append({"run": f"{who}{i}", "ms_per_step": line["ms_per_step"], "value": line["value"], "unit": line["unit"]})
                print(runs[-1], flush=True)
            same.append({k: bool(np.load(os.path.join(tmp, f"parent{i}", k + ".npy")).tobytes() == np.load(os.path.join(tmp, f"new{i}", k + ".npy")).tobytes())
                         for k in ("loss", "log_prob", "bpd")})
        shape = list(np.load(os.path.join(tmp, "new1", "log_prob.npy")).shape)
    stat = lambda who: (lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)})([r["ms_per_step"] for r in runs if r["run"].startswith(who)])
    par, new = stat("parent"), stat("new")
    res = {"what": f"same-box A/B, one GPU call, alternating runs of `python bench.py --gpus 1 --config {C3} --steps 20 --warmup 5 --dump-outputs DIR`: "
                   "parent = the commit before the counted PAConv path (its library through FCFLOW_LIB), new = this build",
           "runs": runs, "parent_ms_per_step": par, "new_ms_per_step": new,
           "new_median_inside_parent_min_max": bool(par["min"] <= new["median"] <= par["max"]), "log_prob_shape": shape, "byte_identical": same}
    print(json.dumps(res), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/paconv_counts.json, with --ab-parent profiles/paconv_counts_ab_parent.json")
    ap.add_argument("--ab-parent", metavar="PARENT_LIB", default=None)
    a = ap.parse_args()
    if a.ab_parent is not None:
        ab_parent(a.ab_parent, a.out or os.path.join(ROOT, "profiles", "paconv_counts_ab_parent.json"))
    else:
        measure(a.out or os.path.join(ROOT, "profiles", "paconv_counts.json"))
