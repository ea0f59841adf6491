#!/usr/bin/env python3
"""Volume-query throughput on the bench's C3 scene (depth-11 Custom1 terrain): svo_overlap_volumes on one
device with 1 M spheres centred on surface voxels -- the hit voxels of a 1920x1080 flyover frame, drawn with
replacement -- at radii of 1, 4 and 16 leaf voxels (a leaf is 1/64 world unit), for

  any : SVO_OVERLAP_ANY, no contacts -- "is this spot free?"
  k0  : the full count, no contacts
  k8  : the full count and the first 8 contacts

Each writes the summaries and the hit mask (k8: the contacts too).  Events on the caller's stream; warm-up,
then REPS repetitions; medians.  Reported per case: shapes/s, the mean visits and count per shape and the share
of shapes that ran into the default budget.  The summaries of one repetition are checked against the host form
on the first 4,096 shapes.  Measured numbers, not pass/fail bars; profiles/query_bench.json's rays/s are quoted
beside them for context (a ray and a volume are different work).

  python tools/overlap_bench.py [--reps 10] [--shapes 1000000] [--out profiles/overlap_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", type=int, default=1000000)
    ap.add_argument("--max-level", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_bench.json"))
    args = ap.parse_args()
    import torch
    from raytracingtest_amd import HIT_DTYPE, RaytracingMaster, build
    from raytracingtest_amd import overlap as ov
    from raytracingtest_amd.camera import CAMERAS
    from raytracingtest_amd.native_builder import build_sampler_svo

    W, H = 1920, 1080
    n = args.shapes
    svo = build_sampler_svo(4, args.max_level)
    rm = RaytracingMaster(device=0, capacity_nodes=len(svo))
    rm.SetSVOBuffer(svo)
    rm.UpdateShaderParameters(CAMERAS["flyover"](), W, H)
    stream = torch.cuda.Stream()
    sptr = stream.cuda_stream

    # surface voxels: the hit voxels of one frame
    d_hits = torch.zeros(W * H * 24, dtype=torch.uint8, device="cuda")
    d_vox = torch.zeros(W * H, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rm.render_frame(W, H, hits=d_hits.data_ptr(), voxel=d_vox.data_ptr(), stream=sptr)
    stream.synchronize()
    hits = d_hits.cpu().numpy().view(HIT_DTYPE)
    keys = d_vox.cpu().numpy().view(np.uint64)
    on = np.flatnonzero(hits["flags"] & 1)
    rng = np.random.default_rng(3)
    pick = on[rng.integers(0, len(on), n)]
    level = 23 - hits["hit_scale"][pick].astype(np.int64)
    side = 2.0 ** (5 - level)
    xyz = np.stack([(keys[pick] >> np.uint64(21 * k)) & np.uint64(0x1FFFFF) for k in range(3)], axis=1).astype(np.float64)
    centres = (xyz + 0.5) * side[:, None] - 16.0
    leaf = 2.0 ** (5 - args.max_level)

    d_summary = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_contacts = torch.zeros(n * 8 * 16, dtype=torch.uint8, device="cuda")
    d_mask = torch.zeros((n + 63) // 64 * 8, dtype=torch.uint8, device="cuda")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    ref = None
    try:
        with open(os.path.join(ROOT, "profiles", "query_bench.json")) as fh:
            q = json.load(fh)
        ref = {k: v["unordered_Mrays_per_s"] for k, v in q["batches"].items()}
    except (OSError, KeyError, ValueError):
        pass
    out = {"scene": f"C3 (Custom1 depth {args.max_level}, {len(svo)} nodes), spheres on the hit voxels of the {W}x{H} flyover frame",
           "source_digest": build.source_digest(), "shapes": n, "reps": args.reps, "warmup": args.warmup,
           "surface_voxels_in_frame": int(len(on)), "leaf_side_world": leaf,
           "query_bench_unordered_Mrays_per_s": ref, "cases": {}}
    for radius in (1, 4, 16):
        shapes = ov.make_spheres(centres, radius * leaf)
        d_shapes = torch.from_numpy(shapes.view(np.uint8).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        for mode, K, any_hit in (("any", 0, True), ("k0", 0, False), ("k8", 8, False)):
            def run():
                rm.overlap_volumes_device(d_shapes.data_ptr(), n, summary=d_summary.data_ptr(),
                                          contacts=d_contacts.data_ptr() if K else None, hitmask=d_mask.data_ptr(),
                                          max_contacts=K, any_hit=any_hit, stream=sptr)
            times = [timed(run) for _ in range(args.warmup + args.reps)][args.warmup:]
            ms = float(np.median(times))
            s = d_summary.cpu().numpy().view(ov.OVERLAP_DTYPE)
            m = min(n, 4096)
            host = rm.OverlapVolumes(shapes[:m], max_contacts=0, any_hit=any_hit)
            assert host.tobytes() == s[:m].tobytes(), f"radius {radius} {mode}: host and device forms differ"
            case = {"ms": round(ms, 4), "Mshapes_per_s": round(n / ms / 1e3, 2),
                    "mean_visits": round(float(s["visits"].mean()), 2), "max_visits": int(s["visits"].max()),
                    "mean_count": round(float(s["count"].mean()), 2),
                    "touching_share": round(float(((s["flags"] & 1) != 0).mean()), 4),
                    "budget_share": round(float(((s["flags"] & 2) != 0).mean()), 6)}
            out["cases"][f"r{radius}_{mode}"] = case
            print(f"r{radius}_{mode}", json.dumps(case), flush=True)
    rm.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
