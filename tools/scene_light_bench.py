#!/usr/bin/env python3
"""Objects in shadow and light on the bench's C3 scene (depth-11 Custom1 terrain, 1920x1080): what the
scene-aware shadow and light passes (SVO_OPT_SCENE_SHADOWS) cost a frame that shows placed objects, at the
flyover and the Main.unity pose, with tools/objects_bench.py's 1, 4 and 8 placements.

Per object count the settings are: the objects alone, + the directional shadow rays, + 1 / 4 / 8 point
lights, + shadows and 4 lights.  Light j hangs LIGHT_LIFT world units above the primary hit that object j of
objects_bench.py hangs over (so 3 units above the object), with a range of LIGHT_RANGE units.

Timing as objects_bench.py: the whole render of a frame into an RGBA32F device buffer -- the primary launch,
the object pass and the scene-aware passes -- bracketed by events on the render's stream; the settings are
interleaved in one process, ROUNDS rounds of BLOCK launches each at a held view, the first SKIP of a block
dropped.  Reported: the median over all kept launches of a setting, the spread of the per-round medians, and
the cost as a multiple of the same run's frame with the same objects alone.  Not pass/fail numbers.

  python tools/scene_light_bench.py [--rounds 8] [--block 30] [--out profiles/scene_light_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIGHT_LIFT = 6.0
LIGHT_RANGE = 12.0
COLOURS = [(3.0, 2.5, 2.0), (0.5, 2.0, 4.0), (6.0, 1.0, 0.25), (2.0, 3.0, 1.0)]
# (name, shadows, lights)
KINDS = [("alone", False, 0), ("shadows", True, 0), ("L1", False, 1), ("L4", False, 4), ("L8", False, 8), ("both", True, 4)]
COUNTS = [1, 4, 8]


def light_set(points, k):
    return [((float(p[0]), float(p[1]) + LIGHT_LIFT - 3.0, float(p[2])), LIGHT_RANGE, COLOURS[j % len(COLOURS)])
            for j, p in enumerate(points[:k])]


def measure(torch, rm, cam, points, root, w, h, mode, args):
    import objects_bench as ob
    n = w * h
    stream = torch.cuda.Stream()
    sptr = stream.cuda_stream
    d_rgba = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rm.UpdateShaderParameters(cam, w, h)
    settings = [(f"O{c}_{name}", c, sh, nl) for c in COUNTS for name, sh, nl in KINDS]
    times = {s[0]: [] for s in settings}
    rounds = {s[0]: [] for s in settings}
    for r in range(args.rounds + 1):           # round 0: warm-up of every setting's kernels
        order = settings if r % 2 == 0 else settings[::-1]
        for name, c, shadows, n_lights in order:
            rm.SetObjects(ob.object_set(points, c, root))
            rm.SetShadowRays(shadows)
            rm.SetLights(light_set(points, n_lights) if n_lights else None)
            evs = []
            with torch.cuda.stream(stream):
                for _ in range(args.block):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    rm.render_device(w, h, rgba_ptr=d_rgba.data_ptr(), stack_mode=mode, stream=sptr)
                    e1.record(stream)
                    evs.append((e0, e1))
            stream.synchronize()
            ms = np.asarray([a.elapsed_time(b) for a, b in evs], np.float64)[args.skip:]
            if r > 0 and len(ms):
                times[name].extend(ms.tolist())
                rounds[name].append(float(np.median(ms)))
    rm.SetObjects(None)
    rm.SetShadowRays(False)
    rm.SetLights(None)
    rm.forget_stream(sptr)
    out = {}
    for name, c, shadows, n_lights in settings:
        med = float(np.median(times[name]))
        alone = float(np.median(times[f"O{c}_alone"]))
        out[name] = {"n_objects": c, "shadows": shadows, "n_lights": n_lights, "frame_ms_median": round(med, 5),
                     "frame_ms_round_medians_min_max": [round(min(rounds[name]), 5), round(max(rounds[name]), 5)],
                     "launches_timed": len(times[name]), "multiple_of_frame_with_objects_alone": round(med / alone, 3)}
        print(json.dumps({name: out[name]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--block", type=int, default=30)
    ap.add_argument("--skip", type=int, default=10)
    ap.add_argument("--max-level", type=int, default=11)
    ap.add_argument("--model-level", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_light_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scene_light_bench.py measures on a GPU; none is visible, nothing is written")
    import objects_bench as ob
    from raytracingtest_amd import RaytracingMaster, build
    from raytracingtest_amd.camera import CAMERAS
    from raytracingtest_amd.native_builder import build_sampler_svo

    out = {"source_digest": build.source_digest(), "rounds": args.rounds, "block": args.block, "skip": args.skip,
           "object_lift": ob.LIFT, "scale_log2": ob.SCALE_LOG2, "light_lift": LIGHT_LIFT, "light_range": LIGHT_RANGE,
           "method": "events on the render's stream around each svo_render_device into an RGBA32F buffer (primary launch, "
                     "object pass, scene-aware shadow and light passes); settings interleaved, first `skip` launches of "
                     "each block dropped",
           "scenes": {}}
    w, h, mode = 1920, 1080, 0
    svo = build_sampler_svo(4, args.max_level)
    model = build_sampler_svo(4, args.model_level)
    root = len(svo)
    if model.format == 2:   # absolute child pointers: moved with the tree (a v1 pool is uploaded as it is)
        from raytracingtest_amd import SVOData
        first = (model.nodes >> np.uint64(32)) + np.uint64(root)
        model = SVOData(nodes=(first << np.uint64(32)) | (model.nodes & np.uint64(0xFFFFFFFF)), attachments=model.attachments)
    rm = RaytracingMaster(device=0, capacity_nodes=len(svo) + len(model))
    rm.SetSVOBuffer(svo)
    rm.SetSVOBuffer(model, root)
    rm.SetSceneShadows(True)
    for pose in ("flyover", "main"):
        print(f"== C3 depth {args.max_level - 1}, {len(svo)} + {len(model)} nodes, {w}x{h}, {pose}", flush=True)
        cam = CAMERAS[pose]()
        d_rays, d_hits, d_pos = ob.primary(torch, rm, cam, w, h, mode)
        points = ob.anchor_points(d_hits, d_pos, w, h)
        out["scenes"][f"C3_{pose}"] = {"terrain_nodes": len(svo), "model_nodes": len(model), "width": w, "height": h,
                                       "stack_mode": mode, "object_positions": [[round(v, 4) for v in p] for p in points],
                                       "settings": measure(torch, rm, cam, points, root, w, h, mode, args)}
        del d_rays, d_hits, d_pos
    rm.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
