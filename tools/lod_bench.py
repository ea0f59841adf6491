#!/usr/bin/env python3
"""Level of detail on the bench's C3 scene (depth-11 Custom1 terrain, 1920x1080; optionally one C4
pose): the primary kernel's sustained time, the descriptor fetches and where the hits land, for
pixels in {off, 1, 2, 4} (ray_size_coef = lod.pixel_footprint(inv_proj, height, pixels), bias 0) at
the flyover and the Main.unity pose.

Timing: svo_stage_time's per-launch kernel times (HIP events around the primary kernel), the settings
interleaved in one process -- ROUNDS rounds, each visiting every setting once for BLOCK launches at a
held view, of which the first SKIP (the launches whose dispatch order still belongs to the previous
setting: a new pair counts as a camera move) are dropped.  Reported: the median over all kept
launches of a setting, and the spread of the per-round medians (min, max) -- a difference inside that
spread is not a difference.  Not pass/fail numbers.

  python tools/lod_bench.py [--rounds 12] [--block 40] [--c4] [--bench-json FILE ...] [--out profiles/lod_bench.json]

--bench-json: result lines of `python bench.py` runs to record beside the figures (LOD off, this
tree and the parent commit's library alternated by the caller), as `label=path` pairs.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [("off", 0.0), ("1", 1.0), ("2", 2.0), ("4", 4.0)]


def measure(torch, rm, svo, cam, w, h, mode, args):
    from raytracingtest_amd import HIT_DTYPE
    from raytracingtest_amd.lod import lod_hit_is_inner, pixel_footprint
    n = w * h
    _, inv_proj = cam.uniforms(w, h)
    stream = torch.cuda.Stream()
    sptr = stream.cuda_stream
    d_hits = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
    d_fetch = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rm.UpdateShaderParameters(cam, w, h)
    rm.set_kernel_timing(True)
    times = {name: [] for name, _ in SETTINGS}
    rounds = {name: [] for name, _ in SETTINGS}
    for r in range(args.rounds + 1):           # round 0: warm-up of every setting's kernels
        order = SETTINGS if r % 2 == 0 else SETTINGS[::-1]
        for name, px in order:
            rm.SetLod(pixel_footprint(inv_proj, h, px) if px else 0.0, 0.0)
            rm.stage_times()                    # drop what is recorded
            for _ in range(args.block):
                rm.render_device(w, h, hits_ptr=d_hits.data_ptr(), stack_mode=mode, stream=sptr)
            stream.synchronize()
            ms = np.asarray(rm.stage_times(), np.float64)[args.skip:]
            if r > 0 and len(ms):
                times[name].extend(ms.tolist())
                rounds[name].append(float(np.median(ms)))
    rm.set_kernel_timing(False)
    out = {}
    for name, px in SETTINGS:
        coef = pixel_footprint(inv_proj, h, px) if px else 0.0
        rm.SetLod(coef, 0.0)
        rm.render_device(w, h, hits_ptr=d_hits.data_ptr(), stack_mode=mode, stream=sptr)
        rm.count_fetches_device(w, h, d_fetch.data_ptr(), stack_mode=mode, stream=sptr)
        stream.synchronize()
        hits = d_hits.cpu().numpy().view(HIT_DTYPE)
        hit = (hits["flags"] & 1) != 0
        inner = lod_hit_is_inner(svo, hits)
        scales, counts = np.unique(hits["hit_scale"][hit], return_counts=True)
        out[name] = {"ray_size_coef": coef,
                     "kernel_ms_median": round(float(np.median(times[name])), 5),
                     "kernel_ms_round_medians_min_max": [round(min(rounds[name]), 5), round(max(rounds[name]), 5)],
                     "launches_timed": len(times[name]),
                     "fetches_total": int(d_fetch.cpu().numpy().astype(np.int64).sum()),
                     "hits": int(hit.sum()), "inner_share_of_hits": round(float(inner.sum()) / max(int(hit.sum()), 1), 4),
                     "hit_scale_histogram": {int(s): int(c) for s, c in zip(scales, counts)}}
        print(json.dumps({name: out[name]}), flush=True)
    rm.SetLod(0.0, 0.0)
    rm.forget_stream(sptr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--skip", type=int, default=10)
    ap.add_argument("--max-level", type=int, default=11)
    ap.add_argument("--c4", action="store_true", help="also the C4 scene (depth 12, 3840x2160, overview pose, exact stack)")
    ap.add_argument("--bench-json", action="append", default=[], metavar="LABEL=FILE")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lod_bench.json"))
    args = ap.parse_args()
    import torch
    from raytracingtest_amd import RaytracingMaster, build
    from raytracingtest_amd.camera import CAMERAS
    from raytracingtest_amd.native_builder import build_sampler_svo

    out = {"source_digest": build.source_digest(), "rounds": args.rounds, "block": args.block, "skip": args.skip,
           "method": "svo_stage_time kernel ms per launch; settings interleaved, first `skip` launches of each block dropped",
           "scenes": {}}
    scenes = [("C3", args.max_level, 1920, 1080, 0, ("flyover", "main"))]
    if args.c4:
        scenes.append(("C4", 13, 3840, 2160, 1, ("overview",)))
    for label, level, w, h, mode, poses in scenes:
        svo = build_sampler_svo(4, level)
        rm = RaytracingMaster(device=0, capacity_nodes=len(svo))
        rm.SetSVOBuffer(svo)
        for pose in poses:
            print(f"== {label} depth {level - 1}, {len(svo)} nodes, {w}x{h}, {pose}", flush=True)
            out["scenes"][f"{label}_{pose}"] = {"nodes": len(svo), "width": w, "height": h, "stack_mode": mode,
                                               "pixels": measure(torch, rm, svo, CAMERAS[pose](), w, h, mode, args)}
        rm.close()
    runs = {}
    for item in args.bench_json:
        lab, path = item.split("=", 1)
        with open(path) as fh:
            lines = [ln for ln in fh if ln.lstrip().startswith("{")]
        runs.setdefault(lab, []).append(json.loads(lines[-1]))
    if runs:
        out["bench_py_lod_off"] = runs
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
