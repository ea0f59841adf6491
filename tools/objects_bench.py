#!/usr/bin/env python3
"""Placed objects on the bench's C3 scene (depth-11 Custom1 terrain, 1920x1080): what the object pass costs a
frame, at the flyover and the Main.unity pose, with 1, 4 and 8 placed objects against the same run's frame
with none.

The object is one small model -- the same sampler's terrain at depth 8, uploaded once behind the terrain's
pool (a v2 tree's absolute child pointers are moved by its offset) -- placed up to eight times (objects may
share a root): 4-unit cubes (scale_log2 -3), each turned about the vertical by another angle, hanging 3 world
units above eight points of the pose's own frame: the primary hits nearest to the centres of a 4 x 2 grid of
the picture (found on the ray-query API, recorded in the output).  A set of n objects is the first n of them.

Timing: the whole render of a frame into an RGBA32F device buffer -- the primary launch plus, with objects,
the object pass -- bracketed by events on the render's stream.  The settings are interleaved in one process:
ROUNDS rounds, each visiting every setting once for BLOCK launches at a held view, of which the first SKIP
are dropped.  Reported: the median over all kept launches of a setting, the spread of the per-round medians
(min, max), and the cost as a multiple of the same run's frame with no object.  Not pass/fail numbers.

Beside the times: per setting the pixels that show an object and the pixels whose ray walks at least one
object, counted on the scene query (svo_trace_scene), which applies the same rule to the same rays.

  python tools/objects_bench.py [--rounds 12] [--block 40] [--out profiles/objects_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIFT = 3.0
SCALE_LOG2 = -3
SETTINGS = [("off", 0), ("O1", 1), ("O4", 4), ("O8", 8)]


def turn(deg):
    t = np.deg2rad(deg)
    return [[np.cos(t), 0.0, np.sin(t)], [0.0, 1.0, 0.0], [-np.sin(t), 0.0, np.cos(t)]]


def object_set(points, n, root):
    return [(root, SCALE_LOG2, tuple(float(v) for v in p), turn(25.0 * j)) for j, p in enumerate(points[:n])]


def primary(torch, rm, cam, w, h, mode):
    """The frame's camera rays, hit records and positions on the device (the ray-query API)."""
    from raytracingtest_amd.query import camera_rays
    n = w * h
    c2w, inv_proj = cam.uniforms(w, h)
    d_rays = torch.from_numpy(camera_rays(c2w, inv_proj, w, h).view(np.uint8).reshape(-1).copy()).cuda()
    d_hits = torch.zeros(n * 6, dtype=torch.int32, device="cuda")
    d_pos = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rm.trace_rays_device(d_rays.data_ptr(), n, hits=d_hits.data_ptr(), position=d_pos.data_ptr(), stack_mode=mode, raw=True)
    rm.synchronize()
    return d_rays, d_hits, d_pos


def anchor_points(d_hits, d_pos, w, h):
    """Eight world-space points LIFT above the primary hits nearest to the centres of a 4 x 2 grid of the frame."""
    hit = (((d_hits.view(w * h, 6)[:, 1] >> 16) & 1) != 0).cpu().numpy().reshape(h, w)
    pos = d_pos.view(w * h, 4).cpu().numpy().reshape(h, w, 4)
    ys, xs = np.nonzero(hit)
    if len(ys) == 0:
        raise RuntimeError("the frame has no hit pixel to hang an object over")
    points = []
    for r in range(2):
        for c in range(4):
            cy, cx = h * (r + 0.5) / 2.0, w * (c + 0.5) / 4.0
            k = int(np.argmin((ys - cy) ** 2 + (xs - cx) ** 2))
            p = pos[ys[k], xs[k], :3].astype(np.float64) * 0.5   # svo_hit positions are twice the world's
            points.append((p[0], p[1] + LIFT, p[2]))
    return points


def pixel_shares(torch, rm, d_rays, points, root, w, h, mode):
    """Per setting: the pixels that show an object, and those whose ray walks one with the terrain left out."""
    n = w * h
    out = {}
    for name, k in [s for s in SETTINGS if s[1]]:
        d_id = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_id2 = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        objs = object_set(points, k, root)
        rm.trace_scene_device(d_rays.data_ptr(), n, objs, object_id=d_id.data_ptr(), stack_mode=mode, raw=True)
        rm.trace_scene_device(d_rays.data_ptr(), n, objs, object_id=d_id2.data_ptr(), stack_mode=mode, raw=True, terrain=False)
        rm.synchronize()
        out[name] = {"object_pixels": int((d_id > 0).sum()), "object_pixels_without_terrain": int((d_id2 > 0).sum()),
                     "pixels": n}
    return out


def measure(torch, rm, cam, points, root, w, h, mode, args):
    n = w * h
    stream = torch.cuda.Stream()
    sptr = stream.cuda_stream
    d_rgba = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rm.UpdateShaderParameters(cam, w, h)
    times = {s[0]: [] for s in SETTINGS}
    rounds = {s[0]: [] for s in SETTINGS}
    for r in range(args.rounds + 1):           # round 0: warm-up of every setting's kernels
        order = SETTINGS if r % 2 == 0 else SETTINGS[::-1]
        for name, k in order:
            rm.SetObjects(object_set(points, k, root) if k else None)
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
    rm.forget_stream(sptr)
    out = {}
    off = float(np.median(times["off"]))
    for name, k in SETTINGS:
        med = float(np.median(times[name]))
        out[name] = {"n_objects": k, "frame_ms_median": round(med, 5),
                     "frame_ms_round_medians_min_max": [round(min(rounds[name]), 5), round(max(rounds[name]), 5)],
                     "launches_timed": len(times[name]), "multiple_of_off_frame": round(med / off, 3)}
        print(json.dumps({name: out[name]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--skip", type=int, default=10)
    ap.add_argument("--max-level", type=int, default=11)
    ap.add_argument("--model-level", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("objects_bench.py measures on a GPU; none is visible, nothing is written")
    from raytracingtest_amd import RaytracingMaster, build
    from raytracingtest_amd.camera import CAMERAS
    from raytracingtest_amd.native_builder import build_sampler_svo

    out = {"source_digest": build.source_digest(), "rounds": args.rounds, "block": args.block, "skip": args.skip,
           "lift": LIFT, "scale_log2": SCALE_LOG2,
           "method": "events on the render's stream around each svo_render_device into an RGBA32F buffer (primary launch + "
                     "object pass); settings interleaved, first `skip` launches of each block dropped",
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
    for pose in ("flyover", "main"):
        print(f"== C3 depth {args.max_level - 1}, {len(svo)} + {len(model)} nodes, {w}x{h}, {pose}", flush=True)
        cam = CAMERAS[pose]()
        d_rays, d_hits, d_pos = primary(torch, rm, cam, w, h, mode)
        points = anchor_points(d_hits, d_pos, w, h)
        scene = {"terrain_nodes": len(svo), "model_nodes": len(model), "width": w, "height": h, "stack_mode": mode,
                 "object_positions": [[round(v, 4) for v in p] for p in points],
                 "settings": measure(torch, rm, cam, points, root, w, h, mode, args)}
        for name, share in pixel_shares(torch, rm, d_rays, points, root, w, h, mode).items():
            scene["settings"][name].update(share)
        print(json.dumps({"object_pixels": {k: v.get("object_pixels") for k, v in scene["settings"].items()}}), flush=True)
        out["scenes"][f"C3_{pose}"] = scene
        del d_rays, d_hits, d_pos
    rm.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
