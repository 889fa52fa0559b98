"""Time of the two new kernels of the dense change maps on the large scene of the staging tests: 2 x 2 M uniform
points in 54 x 54 x 12 m, the 972 centres of the [3, 3, 4] m grid, 1024 / 2048 samples.  Median of 5 runs after 2 warm-ups, device
synchronisation around each.  No gate: there is no parent to compare with.

    python profiles/dense_change_large.py [--out profiles/dense_change_large.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flowcompare_amd import engine, staging  # noqa: E402

DEV = "cuda:0"
FINAL, CONTEXT, N, M = (3.0, 3.0, 4.0), (4.0, 4.0, 5.0), 1024, 2048


def timed(fn):
    ts = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts[2:]) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "dense_change_large.json"))
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(21)
    ext = torch.tensor([54.0, 54.0, 12.0, 1.0, 1.0, 1.0], device=DEV)
    c0 = (torch.rand(2_000_000, 6, device=DEV, generator=g) * ext).contiguous()
    c1 = (torch.rand(2_000_000, 6, device=DEV, generator=g) * ext).contiguous()
    centers = staging.voxel_centers((0.0, 0.0, 0.0), (54.0, 54.0, 12.0), FINAL, device=DEV)
    st = staging.stage_scene(c0, c1, centers, FINAL, CONTEXT, N, M)
    res = {"points": [c0.shape[0], c1.shape[0]], "centres": centers.shape[0], "voxels_staged": st.voxel.numel(), "samples": [N, M], "runs": "median of 5 after 2"}
    for block in (1024, 256):
        ms, dense = timed(lambda: staging.stage_dense(c1, st, FINAL, centers, block))
        inv = torch.cat((st.inverse["furthest_distance"][:, None], st.inverse["mean"]), 1).contiguous()
        rows32 = dense.rows.to(torch.int32)
        ms_k, _ = timed(lambda: engine.stage_dense_blocks(c1, dense.offsets, rows32, inv, dense.block_offsets, dense.blocks.shape[0], block))
        total = dense.rows.numel()
        res[f"block_{block}"] = {"rows": total, "blocks": dense.blocks.shape[0], "pad_rows": dense.blocks.shape[0] * block - total,
                                 "blocks_bytes": dense.blocks.numel() * 4, "stage_dense_ms": round(ms, 3),
                                 "dense_blocks_launch_with_output_allocation_ms": round(ms_k, 3)}
    lp10 = torch.randn(total, device=DEV, generator=g) * 4.0 - 8.0
    lp00 = torch.randn(st.voxel.numel(), N, device=DEV, generator=g) * 2.0 - 5.0
    ms_c, out = timed(lambda: engine.change_map_ragged(lp10, dense.offsets, lp00, 5.4))
    res["change_map_ragged"] = {"rows": total, "voxels": st.voxel.numel(), "n0": N, "ms": round(ms_c, 3), "changed_rows": int((out[0] > 0).sum())}
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
