"""What staging voxels with sparse context costs and buys, on one GPU.  Median of 5 runs after 2 warm-ups, device
synchronisation around the whole staging on both sides, results torch.equal.  No gate: nothing here is asserted in a test.

  * stage_scene(min_context=256) on the swapped fixture scene of tests/sparse_stage_util.py (M = 1280, N = 64) and on the 2 M-point scene
    of tests/test_gpu_scene_stage.py::test_large_scene (972 centres, context counts 3042 .. 4776, M = 4096, N = 1024), against the only way
    the parent commit can stage the same voxels: a Python loop of staging.stage_pair per voxel with that voxel's own count (two masks over
    the clouds per voxel, as tests/test_gpu_scene_stage.py::_loop_stage).  On the large scene the loop runs on every 15th centre (64 of
    them: the subset of the existing speed floor) and stage_scene is timed on the same 64 and on all 972.
  * fa.scene_change on the fixture scene with and without min_context: wall time and embedder calls.

    python profiles/sparse_stage_measure.py [--out profiles/sparse_stage.json]
    rocprofv3 --kernel-trace --stats -d DIR -o sparse -- python profiles/sparse_stage_measure.py --trace     # kernel times, a run of its own
    python profiles/sparse_stage_measure.py --summarise DIR/sparse_results.db                                # per launch, by workgroups
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
KERNELS = ("fps_ragged_counts_kernel", "stage_pairs_counts_kernel", "fps_ragged_kernel", "co_unit_sphere_kernel")


def timed(fn):
    import torch
    ts = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts[2:]) * 1e3, 3), r


def loop_stage(c0, c1, centers, n, m, min_context):
    """the parent's way: per voxel two torch masks over the whole clouds + staging.stage_pair with the voxel's own count"""
    import torch
    from flowcompare_amd import staging
    fin, ctx = torch.tensor(FINAL, device=DEV), torch.tensor(CONTEXT, device=DEV)
    out = []
    for k in range(centers.shape[0]):
        c = centers[k]
        v1 = c1[((c1[:, :3] >= c - fin / 2).all(1) & (c1[:, :3] <= c + fin / 2).all(1))]
        v0 = c0[((c0[:, :3] >= c - ctx / 2).all(1) & (c0[:, :3] <= c + ctx / 2).all(1))]
        if v0.shape[0] < min_context or v1.shape[0] < n:
            continue
        out.append((k, min(v0.shape[0], m)) + tuple(staging.stage_pair(v0, v1, min(v0.shape[0], m), n)))
    return out


def equal(st, loop):
    import torch
    ok = st.voxel.tolist() == [k for k, *_ in loop] and st.context_counts.tolist() == [c for _, c, *_ in loop]
    for i, (k, c, s0, s1, inv) in enumerate(loop):
        ok = ok and torch.equal(st.extract_0[i, :c], s0) and torch.equal(st.extract_1[i], s1) and bool((st.extract_0[i, c:] == 0).all())
        ok = ok and torch.equal(st.inverse["furthest_distance"][i], inv["furthest_distance"]) and torch.equal(st.inverse["mean"][i], inv["mean"])
    return bool(ok)


def scenes():
    import torch
    import sparse_stage_util as SU
    import scene_stage_util as U
    from flowcompare_amd import staging
    f0, f1 = (torch.from_numpy(c).to(DEV) for c in SU.swapped_scene())
    fc = torch.from_numpy(U.centers_np()).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(21)
    ext = torch.tensor([54.0, 54.0, 12.0, 1.0, 1.0, 1.0], device=DEV)
    l0 = (torch.rand(2_000_000, 6, device=DEV, generator=g) * ext).contiguous()
    l1 = (torch.rand(2_000_000, 6, device=DEV, generator=g) * ext).contiguous()
    lc = staging.voxel_centers((0.0, 0.0, 0.0), (54.0, 54.0, 12.0), FINAL, device=DEV)
    return (f0, f1, fc, 64, 1280), (l0, l1, lc, 1024, 4096)


def measure(out_path):
    import torch
    import flowcompare_amd as fa
    from flowcompare_amd import staging
    (f0, f1, fc, fn, fm), (l0, l1, lc, ln, lm) = scenes()
    res = {"runs": "median of 5 after 2 warm-ups, device synchronisation around the whole staging", "min_context": 256}

    def pair(name, c0, c1, centers, n, m):
        ms_new, st = timed(lambda: staging.stage_scene(c0, c1, centers, FINAL, CONTEXT, n, m, min_context=256))
        ms_loop, loop = timed(lambda: loop_stage(c0, c1, centers, n, m, 256))
        ms_none, st_none = timed(lambda: staging.stage_scene(c0, c1, centers, FINAL, CONTEXT, n, m))
        cc = st.context_counts
        res[name] = {"points": [c0.shape[0], c1.shape[0]], "centres": centers.shape[0], "samples": [n, m], "voxels_staged": st.voxel.numel(),
                     "voxels_sparse": int((cc < m).sum()), "context_counts": [int(cc.min()), int(cc.max())],
                     "voxels_staged_without_min_context": st_none.voxel.numel(), "stage_scene_min_context_ms": ms_new,
                     "stage_scene_without_min_context_ms": ms_none, "stage_pair_loop_ms": ms_loop, "ratio": round(ms_loop / ms_new, 1),
                     "results_equal": equal(st, loop)}
        print(name, json.dumps(res[name]), flush=True)

    pair("fixture_swapped", f0, f1, fc, fn, fm)
    pair("large_64_centres", l0, l1, lc[torch.arange(0, 972, 15)[:64]].contiguous(), ln, lm)
    ms_all, st = timed(lambda: staging.stage_scene(l0, l1, lc, FINAL, CONTEXT, ln, lm, min_context=256))
    ms_all_none, st_none = timed(lambda: staging.stage_scene(l0, l1, lc, FINAL, CONTEXT, ln, lm))
    res["large_all_centres"] = {"centres": 972, "samples": [ln, lm], "voxels_staged": st.voxel.numel(), "voxels_sparse": int((st.context_counts < lm).sum()),
                                "context_box_counts": [int(st.count_0.min()), int(st.count_0.max())], "stage_scene_min_context_ms": ms_all,
                                "voxels_staged_without_min_context": st_none.voxel.numel(), "stage_scene_without_min_context_ms": ms_all_none}
    print("large_all_centres", json.dumps(res["large_all_centres"]), flush=True)

    # scene_change on the fixture scene: wall time and embedder calls, with and without min_context
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=2, sample_size=fn, n_samples_context=fm)
    cfg["final_voxel_size"], cfg["context_voxel_size"] = FINAL, CONTEXT
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    calls = [0]
    md["input_embedder"].register_forward_hook(lambda *a: calls.__setitem__(0, calls[0] + 1))
    res["scene_change_fixture"] = {"config": "c4_dgcnn_attn_extra_affine, 2 flow layers", "voxels_per_batch": 16}
    for name, kw in (("without_min_context", {}), ("min_context_256", {"min_context": 256})):
        for dense in (False, True):
            def run():
                torch.manual_seed(11)
                calls[0] = 0
                return fa.scene_change(f0, f1, md, cfg, fc, ground_height=0.25, voxels_per_batch=16, dense=dense, **kw)
            ms, (out, st) = timed(run)
            res["scene_change_fixture"][f"{name}_{'dense' if dense else 'sampled'}"] = {
                "ms": ms, "embedder_calls": calls[0], "voxels": st.voxel.numel(), "points_scored": int(torch.isfinite(out).sum())}
    print("scene_change_fixture", json.dumps(res["scene_change_fixture"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def trace():
    """the staging calls alone, for rocprofv3 --kernel-trace: fixture scene (grids of 32 workgroups) and large scene (972)"""
    import torch
    from flowcompare_amd import staging
    (f0, f1, fc, fn, fm), (l0, l1, lc, ln, lm) = scenes()
    for _ in range(5):
        staging.stage_scene(f0, f1, fc, FINAL, CONTEXT, fn, fm, min_context=256)
        staging.stage_scene(l0, l1, lc, FINAL, CONTEXT, ln, lm, min_context=256)
        staging.stage_scene(l0, l1, lc, FINAL, CONTEXT, ln, 2048)                  # the path without counts beside it: every voxel has >= 2048
    torch.cuda.synchronize()


def summarise(path, out_path):
    """rocprofv3's kernel trace (the `kernels` view of its results .db) -> per-launch microseconds of the staging kernels, grouped by kernel
    and number of workgroups"""
    import sqlite3
    rows = sqlite3.connect(path).execute("select name, grid_x, workgroup_x, end - start from kernels").fetchall()
    groups = {}
    for name, grid, wg, ns in rows:
        short = next((k for k in KERNELS if f"fc::{k}(" in name or name in (k, f"fc::{k}") or f"{len(k)}{k}E" in name), None)
        if short is not None:
            groups.setdefault((short, grid // max(wg, 1)), []).append(ns / 1e3)
    res = [{"kernel": k, "workgroups": wg, "launches": len(v), "us_median": round(statistics.median(v), 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1)}
           for (k, wg), v in sorted(groups.items())]
    print(json.dumps(res, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/sparse_stage.json; with --summarise: print only")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV")
    a = ap.parse_args()
    if a.summarise is not None:
        summarise(a.summarise, a.out)
    elif a.trace:
        trace()
    else:
        measure(a.out or os.path.join(ROOT, "profiles", "sparse_stage.json"))
