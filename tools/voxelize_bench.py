#!/usr/bin/env python3
"""What the mesh builder (svob_build_mesh) costs, per kernel and end to end, beside the sampler pass on the same
grid.  Recorded, not pass/fail.

Cases, all at max_level 11 (a 1024^3 grid, 8 slabs of 128 planes at the default budget):
  ico7      an icosphere of 7 subdivisions, 327,680 triangles of about 3 voxels a side
  bigtiny   200,000 small triangles (up to 6 voxels across here) plus 8 that span the grid (the load-balance shape)
  tiny      bigtiny's 200,000 small triangles alone: the difference is what the 8 spanning ones cost
  sphere    svob_build_sampler(SVOB_SPHERE, 11): the existing leaf pass on the same grid, the yardstick.  The
            reference's sphere lies outside the cube [1,2]^3, so it has no leaves: the figure is the dense
            sign + classify pass over 1026^2 x 1024 cells alone, with no list, sort or layout behind it

Per case: the end-to-end wall time of the build call (upload, kernels, read-back, host sort, host layout), the
median of `--repeats` runs after one warm-up, and for the meshes one more run with svob_mesh_profile on, which
gives the device-event time of each kernel summed over the slabs (that run waits after every launch, so its own
wall time is not reported).

  python tools/voxelize_bench.py [--repeats 5] [--out profiles/voxelize_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats):
    fn()   # warm-up: the first call loads the code objects
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-level", type=int, default=11)
    ap.add_argument("--subdivisions", type=int, default=7)
    ap.add_argument("--small", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxelize_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("voxelize_bench.py measures on a GPU; none is visible, nothing is written")
    from raytracingtest_amd import build
    from raytracingtest_amd import native_builder as nb
    from tests import voxelize_util as vu

    ml = args.max_level
    big_pos, big_tri = vu.bigtiny(args.small, n_big=8)
    meshes = {"ico7": vu.icosphere(args.subdivisions), "bigtiny": (big_pos, big_tri),
              "tiny": (big_pos, big_tri[8:])}
    out = {"source_digest": build.source_digest("libsvo_build.so"), "max_level": ml, "repeats": args.repeats,
           "method": "wall time of the whole build call, median of `repeats` after a warm-up; per-kernel device-event sums "
                     "from one more run with svob_mesh_profile on",
           "cases": {}}
    for name, (pos, tri) in meshes.items():
        (svo, rep, stats), ms = timed(lambda: nb.build_mesh_svo(pos, tri, ml, report=True), args.repeats)
        nb.mesh_profile(True)
        nb.build_mesh_svo(pos, tri, ml)
        kernels = nb.mesh_profile(False)
        case = {"triangles": len(tri), "leaves": int(svo.n_leaves), "nodes": len(svo), "report": rep, "stats": stats,
                "build_ms_median": round(float(np.median(ms)), 3), "build_ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
                "kernel_ms": {k: round(v, 4) for k, v in kernels.items()},
                "kernel_ms_total": round(sum(kernels.values()), 4)}
        out["cases"][name] = case
        print(json.dumps({name: case}), flush=True)
    svo, ms = timed(lambda: nb.build_sampler_svo(nb.SPHERE, ml), args.repeats)
    out["cases"]["sphere"] = {"leaves": int(svo.n_leaves), "nodes": len(svo), "build_ms_median": round(float(np.median(ms)), 3),
                              "build_ms_min_max": [round(min(ms), 3), round(max(ms), 3)]}
    print(json.dumps({"sphere": out["cases"]["sphere"]}), flush=True)
    b, t = out["cases"]["bigtiny"]["kernel_ms"], out["cases"]["tiny"]["kernel_ms"]
    out["spanning_triangles"] = {
        "overlap_ms_with": b["overlap"], "overlap_ms_without": t["overlap"],
        "share_of_bigtiny_overlap": round(1.0 - t["overlap"] / b["overlap"], 4) if b["overlap"] > 0 else None,
        "share_of_bigtiny_kernels": round(1.0 - sum(t.values()) / sum(b.values()), 4) if sum(b.values()) > 0 else None,
        "candidates_with": out["cases"]["bigtiny"]["stats"]["candidates"],
        "candidates_without": out["cases"]["tiny"]["stats"]["candidates"]}
    print(json.dumps({"spanning_triangles": out["spanning_triangles"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
