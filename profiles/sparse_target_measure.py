"""What keeping voxels with few target points costs and buys, on one GPU.  Median (min .. max) of 5 runs after 2
warm-ups, the host clock around a device synchronisation on both sides, results torch.equal.  No gate: nothing here is asserted in a test.

  * stage_scene(min_target=64) on the fixture scene of tests/scene_stage_util.py (M = 1024, N = 720; two final boxes of cloud 1 hold 89 and 103
    points) and on the 2 M-point scene of tests/test_gpu_scene_stage.py::test_large_scene with cloud 1 thinned to 1/8 where x > 45, y > 45
    (972 centres, M = 2048: every context box holds more, N = 1024), against the same call without min_target (which stages fewer voxels) and against the only way the
    parent commit can stage the same voxels: a Python loop of staging.stage_pair per voxel with that voxel's own target count.  On the large
    scene the loop runs on 64 centres (the 27 thinned ones and 37 others) and stage_scene is timed on the same 64 and on all 972.
  * fa.scene_change on the fixture scene, sampled and dense, with and without min_target: wall time and points scored.

    python profiles/sparse_target_measure.py [--out profiles/sparse_target.json]
    rocprofv3 --kernel-trace --stats -d DIR -o target -- python profiles/sparse_target_measure.py --trace     # kernel times, a run of its own
    python profiles/sparse_target_measure.py --summarise DIR/.../target_results.db [--out profiles/sparse_target_kernels.json]
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
MIN_TARGET = 64
# (the ragged FPS kernels are left out: context and target launches of one grid differ in m, which the trace does not carry)
KERNELS = ("stage_pairs_counts2_kernel", "stage_pairs_counts_kernel", "co_unit_sphere_kernel", "change_map_counts_kernel", "change_map_kernel", "inf_stats_counts_kernel", "inf_stats_kernel")


def timed(fn):
    import torch
    ts = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ms = [t * 1e3 for t in ts[2:]]
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}, r


def loop_stage(c0, c1, centers, n, m, min_target):
    """the parent's way: per voxel two torch masks over the whole clouds + staging.stage_pair with the voxel's own target count"""
    import torch
    from flowcompare_amd import staging
    fin, ctx = torch.tensor(FINAL, device=DEV), torch.tensor(CONTEXT, device=DEV)
    out = []
    for k in range(centers.shape[0]):
        c = centers[k]
        v1 = c1[((c1[:, :3] >= c - fin / 2).all(1) & (c1[:, :3] <= c + fin / 2).all(1))]
        v0 = c0[((c0[:, :3] >= c - ctx / 2).all(1) & (c0[:, :3] <= c + ctx / 2).all(1))]
        if v0.shape[0] < m or v1.shape[0] < min_target:
            continue
        out.append((k, min(v1.shape[0], n)) + tuple(staging.stage_pair(v0, v1, m, min(v1.shape[0], n))))
    return out


def equal(st, loop):
    import torch
    ok = st.voxel.tolist() == [k for k, *_ in loop] and st.target_counts.tolist() == [t for _, t, *_ in loop]
    for i, (k, t, s0, s1, inv) in enumerate(loop):
        ok = ok and torch.equal(st.extract_0[i], s0) and torch.equal(st.extract_1[i, :t], s1) and bool((st.extract_1[i, t:] == 0).all())
        ok = ok and torch.equal(st.inverse["furthest_distance"][i], inv["furthest_distance"]) and torch.equal(st.inverse["mean"][i], inv["mean"])
    return bool(ok)


def scenes():
    import torch
    import scene_stage_util as U
    from flowcompare_amd import staging
    f0, f1 = (torch.from_numpy(c).to(DEV) for c in U.scene())
    fc = torch.from_numpy(U.centers_np()).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(21)
    ext = torch.tensor([54.0, 54.0, 12.0, 1.0, 1.0, 1.0], device=DEV)
    l0 = (torch.rand(2_000_000, 6, device=DEV, generator=g) * ext).contiguous()
    l1 = (torch.rand(2_000_000, 6, device=DEV, generator=g) * ext).contiguous()
    keep = ~((l1[:, 0] > 45) & (l1[:, 1] > 45)) | (torch.rand(l1.shape[0], device=DEV, generator=g) < 0.125)
    l1 = l1[keep].contiguous()
    lc = staging.voxel_centers((0.0, 0.0, 0.0), (54.0, 54.0, 12.0), FINAL, device=DEV)
    return (f0, f1, fc, 720, 1024), (l0, l1, lc, 1024, 2048)


def measure(out_path):
    import torch
    import flowcompare_amd as fa
    from flowcompare_amd import staging
    (f0, f1, fc, fn, fm), (l0, l1, lc, ln, lm) = scenes()
    res = {"runs": "median (min .. max) of 5 after 2 warm-ups, host clock around a device synchronisation, milliseconds", "min_target": MIN_TARGET}

    def pair(name, c0, c1, centers, n, m):
        ms_new, st = timed(lambda: staging.stage_scene(c0, c1, centers, FINAL, CONTEXT, n, m, min_target=MIN_TARGET))
        ms_loop, loop = timed(lambda: loop_stage(c0, c1, centers, n, m, MIN_TARGET))
        ms_none, st_none = timed(lambda: staging.stage_scene(c0, c1, centers, FINAL, CONTEXT, n, m))
        tc = st.target_counts
        res[name] = {"points": [c0.shape[0], c1.shape[0]], "centres": centers.shape[0], "samples": [n, m], "voxels_staged": st.voxel.numel(),
                     "voxels_thin": int((tc < n).sum()), "target_counts": [int(tc.min()), int(tc.max())],
                     "voxels_staged_without_min_target": st_none.voxel.numel(), "stage_scene_min_target_ms": ms_new,
                     "stage_scene_without_min_target_ms": ms_none, "stage_pair_loop_ms": ms_loop,
                     "ratio_of_medians": round(ms_loop["median"] / ms_new["median"], 1), "results_equal": equal(st, loop)}
        print(name, json.dumps(res[name]), flush=True)

    pair("fixture", f0, f1, fc, fn, fm)
    c1_fin = staging.voxel_counts(l1, lc, FINAL)
    thin = torch.nonzero(c1_fin < ln).flatten()
    others = torch.nonzero(c1_fin >= ln).flatten()[::26][:64 - thin.numel()]
    subset = torch.cat((thin, others)).sort().values
    pair("large_64_centres", l0, l1, lc[subset].contiguous(), ln, lm)
    ms_all, st = timed(lambda: staging.stage_scene(l0, l1, lc, FINAL, CONTEXT, ln, lm, min_target=MIN_TARGET))
    ms_all_none, st_none = timed(lambda: staging.stage_scene(l0, l1, lc, FINAL, CONTEXT, ln, lm))
    res["large_all_centres"] = {"points": [l0.shape[0], l1.shape[0]], "centres": lc.shape[0], "samples": [ln, lm], "voxels_staged": st.voxel.numel(),
                                "voxels_thin": int((st.target_counts < ln).sum()), "final_box_counts": [int(st.count_1.min()), int(st.count_1.max())],
                                "stage_scene_min_target_ms": ms_all, "voxels_staged_without_min_target": st_none.voxel.numel(),
                                "stage_scene_without_min_target_ms": ms_all_none}
    print("large_all_centres", json.dumps(res["large_all_centres"]), flush=True)

    # scene_change on the fixture scene: wall time and points scored, with and without min_target
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=2, sample_size=fn, n_samples_context=fm)
    cfg["final_voxel_size"], cfg["context_voxel_size"] = FINAL, CONTEXT
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    res["scene_change_fixture"] = {"config": "c4_dgcnn_attn_extra_affine, 2 flow layers", "voxels_per_batch": 16, "points_of_cloud_1": f1.shape[0]}
    for name, kw in (("without_min_target", {}), (f"min_target_{MIN_TARGET}", {"min_target": MIN_TARGET})):
        for dense in (False, True):
            def run():
                torch.manual_seed(11)
                return fa.scene_change(f0, f1, md, cfg, fc, ground_height=0.25, voxels_per_batch=16, dense=dense, **kw)
            ms, (out, st) = timed(run)
            res["scene_change_fixture"][f"{name}_{'dense' if dense else 'sampled'}"] = {
                "ms": ms, "voxels": st.voxel.numel(), "points_scored": int(torch.isfinite(out).sum())}
    print("scene_change_fixture", json.dumps(res["scene_change_fixture"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def trace():
    """the new kernels beside their namesakes, for rocprofv3 --kernel-trace: staging on the fixture scene (32 workgroups) and the large scene
    (972), the change map on one chunk of 16 voxels x 720 slots"""
    import torch
    from flowcompare_amd import change, staging
    (f0, f1, fc, fn, fm), (l0, l1, lc, ln, lm) = scenes()
    g = torch.Generator().manual_seed(1)
    lp10, lp00 = (torch.randn(16, 720, generator=g) * 3 - 5).to(DEV), (torch.randn(16, 720, generator=g) * 2 - 3).to(DEV)
    c1 = torch.tensor([89, 103] + [720] * 14, dtype=torch.int32, device=DEV)
    c0 = torch.full((16,), 720, dtype=torch.int32, device=DEV)
    for _ in range(5):
        staging.stage_scene(f0, f1, fc, FINAL, CONTEXT, fn, fm, min_target=MIN_TARGET)
        staging.stage_scene(f0, f1, fc, FINAL, CONTEXT, 512, fm, min_context=fm)       # stage_pairs_counts_kernel beside it
        staging.stage_scene(l0, l1, lc, FINAL, CONTEXT, ln, lm, min_target=MIN_TARGET)
        staging.stage_scene(l0, l1, lc, FINAL, CONTEXT, ln, lm)
        change.log_prob_to_change_counts(lp10, c1, lp00, c0, 1.0)
        change.log_prob_to_change(lp10, lp00, 1.0)
    torch.cuda.synchronize()


def summarise(path, out_path):
    """rocprofv3's kernel trace (the `kernels` view of its results .db) -> per-launch microseconds, grouped by kernel and number of workgroups"""
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
    ap.add_argument("--out", default=None, help="default: profiles/sparse_target.json; with --summarise: print only")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_DB")
    a = ap.parse_args()
    if a.summarise is not None:
        summarise(a.summarise, a.out)
    elif a.trace:
        trace()
    else:
        measure(a.out or os.path.join(ROOT, "profiles", "sparse_target.json"))
