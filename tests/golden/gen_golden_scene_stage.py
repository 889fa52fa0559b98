#!/usr/bin/env python3
"""Golden vectors for the staging of whole scene pairs, produced by RUNNING THE REFERENCE's own functions on the
synthetic scene of tests/scene_stage_util.py (two clouds from seeds, tests/golden/synth.py; only outputs are stored):

  * `utils.get_all_voxel_centers` (utils.py:436-444): the centre grid;
  * `utils.get_voxel(..., return_mask=True)` (utils.py:135-142) for both clouds and both box sizes: member lists as int32 row
    numbers + offsets (key m_<cloud>_<final|context>_rows / _offsets);
  * `utils.co_unit_sphere` (utils.py:271-280), fp64 and fp32, on every valid pair once FPS has picked the rows (xyz columns only: the
    colour columns pass through untouched).

FPS itself is PARITY UNPINNED at reference level: torch_cluster (torch-cluster==1.5.9 in the reference's environment.yml) is not
available here, so its published algorithm as restated in oracle/staging_oracle.py::fps picks the rows; the picks are not stored.
The reference's modules are imported with the same stubs as gen_golden_staging.py; nothing of the reference is copied.

Usage: python tests/golden/gen_golden_scene_stage.py   (writes tests/golden/scene_stage_members.npz, scene_stage_sphere.npz)
"""
import os
import sys
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    sys.path.insert(0, p)

import numpy as np
import torch

import scene_stage_util as U

REF = "/root/reference"


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


_stub("laspy")
sys.modules["laspy"].file = _stub("laspy.file", File=object)
for n in ("open3d", "dash_core_components", "dash_html_components", "pykeops", "pointops_cuda"):
    _stub(n)
_stub("pykeops.torch", Vi=None, Vj=None)
sys.path.insert(0, REF)
import utils as ref_utils  # noqa: E402


def main():
    c0, c1 = U.scene()
    clouds = {"c0": torch.from_numpy(c0), "c1": torch.from_numpy(c1)}
    sizes = {"final": torch.tensor(U.FINAL), "context": torch.tensor(U.CONTEXT)}
    centers = ref_utils.get_all_voxel_centers(torch.tensor(U.START), torch.tensor(U.END), sizes["final"])
    mem = {"centers": centers.numpy()}
    lists = {}
    for cn, cloud in clouds.items():
        for sn, size in sizes.items():
            per = [torch.nonzero(ref_utils.get_voxel(cloud, c, size, return_mask=True)).flatten().numpy().astype(np.int32) for c in centers]
            off = np.zeros(len(per) + 1, dtype=np.int64)
            off[1:] = np.cumsum([len(p) for p in per])
            mem[f"m_{cn}_{sn}_offsets"], mem[f"m_{cn}_{sn}_rows"] = off, np.concatenate(per)
            lists[cn, sn] = per

    sph = {"voxel": [], "e0_f64": [], "e1_f64": [], "e0_f32": [], "e1_f32": [], "far_f64": [], "mean_f64": [], "far_f32": [], "mean_f32": []}
    for k in range(len(centers)):
        m0, m1 = lists["c0", "context"][k], lists["c1", "final"][k]
        if len(m0) < U.N_CONTEXT or len(m1) < U.N_SAMPLES:            # the loader's rule, ams_voxel_loader.py:240
            continue
        v0, v1 = ref_utils.get_voxel(clouds["c0"], centers[k], sizes["context"]), ref_utils.get_voxel(clouds["c1"], centers[k], sizes["final"])
        s0, s1 = v0[torch.from_numpy(U.fps_first(v0.numpy(), U.N_CONTEXT))], v1[torch.from_numpy(U.fps_first(v1.numpy(), U.N_SAMPLES))]
        sph["voxel"].append(k)
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            a, b, inv = ref_utils.co_unit_sphere(s0.to(dt), s1.to(dt), return_inverse=True)
            sph[f"e0_{tag}"].append(a[:, :3].numpy()); sph[f"e1_{tag}"].append(b[:, :3].numpy())
            sph[f"far_{tag}"].append(inv["furthest_distance"].numpy()); sph[f"mean_{tag}"].append(inv["mean"].numpy())
    sph = {k: np.stack(v) for k, v in sph.items()}
    # two files, each below the largest fixture already committed: the fp32 run travels with the member lists
    np.savez_compressed(os.path.join(HERE, "scene_stage_members.npz"), **mem, **{k: v for k, v in sph.items() if k.endswith("f32")})
    np.savez_compressed(os.path.join(HERE, "scene_stage_sphere.npz"), **{k: v for k, v in sph.items() if not k.endswith("f32")})
    cnt = np.diff(mem["m_c1_final_offsets"]), np.diff(mem["m_c0_context_offsets"])
    print(f"{len(centers)} centres, {len(sph['voxel'])} valid; target counts {sorted(cnt[0])[:3]} .. {cnt[0].max()}, context {cnt[1].min()} .. {cnt[1].max()}; "
          f"{sum(v.size for k, v in mem.items() if k.endswith('rows'))} member rows")
    for f in ("scene_stage_members.npz", "scene_stage_sphere.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
