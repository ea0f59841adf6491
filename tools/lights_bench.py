#!/usr/bin/env python3
"""Point lights on the bench's C3 scene (depth-11 Custom1 terrain, 1920x1080): what the light pass costs a
frame, at the flyover and the Main.unity pose, with 1, 4 and 8 lights of a small range (8 world units) and a
scene-wide one (64), against the lights-off frame.

The lights of a pose hang 1.5 world units above eight points of its own frame: the primary hits nearest to
the centres of a 4 x 2 grid of the picture (found on the ray-query API, recorded in the output).  A set of n
lights is the first n of them; every light has colour (2, 2, 2) and casts shadows.

Timing: the whole render of a frame into an RGBA32F device buffer -- the primary launch plus, with lights
on, the hit list's build and the pass -- bracketed by events on the render's stream.  The settings are
interleaved in one process: ROUNDS rounds, each visiting every setting once for BLOCK launches at a held
view, of which the first SKIP are dropped.  Reported: the median over all kept launches of a setting, the
spread of the per-round medians (min, max), and the cost as a multiple of the same run's off frame.  Not
pass/fail numbers.

Beside the times: per setting the shadow rays the pass traces (pairs of hit pixel and light that are facing
and in range) and the share of them that reach the light, counted on the ray-query API (svo_trace_rays ->
svo_light_rays -> svo_trace_rays), which traces the same rays.

  python tools/lights_bench.py [--rounds 12] [--block 40] [--settings off,L4_r8] [--bench-json LABEL=FILE ...]
                              [--out profiles/lights_bench.json]

--bench-json: result lines of `python bench.py` runs to record beside the figures (lights off, this tree
and the parent commit's library alternated by the caller), as `label=path` pairs.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLOUR = (2.0, 2.0, 2.0)
LIFT = 1.5
SETTINGS = [("off", 0, 0.0)] + [(f"L{n}_r{int(r)}", n, r) for r in (8.0, 64.0) for n in (1, 4, 8)]


def light_set(points, n, rng):
    return [(tuple(float(v) for v in p), rng, COLOUR) for p in points[:n]]


def primary(torch, rm, cam, w, h, mode):
    """The frame's camera rays, hit records, keys and positions on the device (the ray-query API)."""
    from raytracingtest_amd.query import camera_rays
    n = w * h
    c2w, inv_proj = cam.uniforms(w, h)
    d_rays = torch.from_numpy(camera_rays(c2w, inv_proj, w, h).view(np.uint8).reshape(-1).copy()).cuda()
    d_hits = torch.zeros(n * 6, dtype=torch.int32, device="cuda")
    d_vox = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_pos = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rm.trace_rays_device(d_rays.data_ptr(), n, hits=d_hits.data_ptr(), voxel=d_vox.data_ptr(), position=d_pos.data_ptr(),
                         stack_mode=mode, raw=True)
    rm.synchronize()
    return d_rays, d_hits, d_vox, d_pos


def light_points(d_hits, d_pos, w, h):
    """Eight world-space points LIFT above the primary hits nearest to the centres of a 4 x 2 grid of the frame."""
    hit = (((d_hits.view(w * h, 6)[:, 1] >> 16) & 1) != 0).cpu().numpy().reshape(h, w)
    pos = d_pos.view(w * h, 4).cpu().numpy().reshape(h, w, 4)
    ys, xs = np.nonzero(hit)
    if len(ys) == 0:
        raise RuntimeError("the frame has no hit pixel to hang a light over")
    points = []
    for r in range(2):
        for c in range(4):
            cy, cx = h * (r + 0.5) / 2.0, w * (c + 0.5) / 4.0
            k = int(np.argmin((ys - cy) ** 2 + (xs - cx) ** 2))
            p = pos[ys[k], xs[k], :3].astype(np.float64) * 0.5   # svo_hit positions are twice the world's
            points.append((p[0], p[1] + LIFT, p[2]))
    return points


def ray_shares(torch, rm, prim, points, w, h, mode):
    """Per setting: the primary hits, the shadow rays traced and the share of them that reach the light."""
    d_rays, d_hits, d_vox, _ = prim
    n = w * h
    hits = int((((d_hits.view(n, 6)[:, 1] >> 16) & 1) != 0).sum())
    out = {}
    for name, k, rng in [s for s in SETTINGS if s[1]]:
        d_out = torch.zeros(n * k * 32, dtype=torch.uint8, device="cuda")
        d_hits2 = torch.zeros(n * k * 6, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rm.light_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), d_vox.data_ptr(), d_out.data_ptr(), light_set(points, k, rng),
                             raw=True)
        rm.trace_rays_device(d_out.data_ptr(), n * k, hits=d_hits2.data_ptr(), stack_mode=mode)
        rm.synchronize()
        flags = (d_hits2.view(n * k, 6)[:, 1] >> 16) & 0xFFFF
        traced = int(((flags & 0x10) == 0).sum())
        lit = int(((flags & 0x11) == 0).sum())
        out[name] = {"primary_hits": hits, "shadow_rays": traced, "rays_per_hit_pixel": round(traced / max(hits, 1), 4),
                     "lit_share": round(lit / max(traced, 1), 4)}
        del d_out, d_hits2
    return out


def measure(torch, rm, cam, points, w, h, mode, args):
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
        for name, k, rng in order:
            rm.SetLights(light_set(points, k, rng) if k else None)
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
    rm.SetLights(None)
    rm.forget_stream(sptr)
    out = {}
    off = float(np.median(times["off"]))
    for name, k, rng in SETTINGS:
        med = float(np.median(times[name]))
        out[name] = {"n_lights": k, "range": rng, "frame_ms_median": round(med, 5),
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
    ap.add_argument("--settings", default="", help="comma-separated subset of the settings (off is always kept)")
    ap.add_argument("--bench-json", action="append", default=[], metavar="LABEL=FILE")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lights_bench.json"))
    args = ap.parse_args()
    if args.settings:
        keep = set(args.settings.split(",")) | {"off"}
        SETTINGS[:] = [s for s in SETTINGS if s[0] in keep]
    import torch
    from raytracingtest_amd import RaytracingMaster, build
    from raytracingtest_amd.camera import CAMERAS
    from raytracingtest_amd.native_builder import build_sampler_svo

    out = {"source_digest": build.source_digest(), "rounds": args.rounds, "block": args.block, "skip": args.skip,
           "colour": list(COLOUR), "lift": LIFT,
           "method": "events on the render's stream around each svo_render_device into an RGBA32F buffer (primary launch + "
                     "light pass); settings interleaved, first `skip` launches of each block dropped",
           "scenes": {}}
    w, h, mode = 1920, 1080, 0
    svo = build_sampler_svo(4, args.max_level)
    rm = RaytracingMaster(device=0, capacity_nodes=len(svo))
    rm.SetSVOBuffer(svo)
    for pose in ("flyover", "main"):
        print(f"== C3 depth {args.max_level - 1}, {len(svo)} nodes, {w}x{h}, {pose}", flush=True)
        cam = CAMERAS[pose]()
        prim = primary(torch, rm, cam, w, h, mode)
        points = light_points(prim[1], prim[3], w, h)
        scene = {"nodes": len(svo), "width": w, "height": h, "stack_mode": mode,
                 "light_positions": [[round(v, 4) for v in p] for p in points],
                 "settings": measure(torch, rm, cam, points, w, h, mode, args)}
        for name, share in ray_shares(torch, rm, prim, points, w, h, mode).items():
            scene["settings"][name].update(share)
        print(json.dumps({"rays_per_hit_pixel": {k: v.get("rays_per_hit_pixel") for k, v in scene["settings"].items()}}), flush=True)
        out["scenes"][f"C3_{pose}"] = scene
        del prim
    rm.close()
    runs = {}
    for item in args.bench_json:
        lab, path = item.split("=", 1)
        with open(path) as fh:
            lines = [ln for ln in fh if ln.lstrip().startswith("{")]
        runs.setdefault(lab, []).append(json.loads(lines[-1]))
    if runs:
        out["bench_py_lights_off"] = runs
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
