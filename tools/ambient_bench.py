#!/usr/bin/env python3
"""The ambient term on the bench's C3 scene (depth-11 Custom1 terrain, 1920x1080): what the ambient
pass costs a frame, at the flyover and the Main.unity pose, for the settings off, N = 4, 8, 16 at
radius 8 and N = 4 at radius inf (ambient 0.5, 0.75, 1.0, variant 0) -- and, through the same bracket,
a reflection frame at the default setting (specular 0.5, 0.25, 0.75, 7 bounces; the term off).

Timing: the whole render of a frame into an RGBA32F device buffer -- the primary launch plus, with
the term on, the hit list's build and the pass -- bracketed by events on the render's stream.  The
settings are interleaved in one process: ROUNDS rounds, each visiting every setting once for BLOCK
launches at a held view, of which the first SKIP are dropped.  Reported: the median over all kept
launches of a setting, the spread of the per-round medians (min, max), and the cost as a multiple of
the same run's off frame.  Not pass/fail numbers.

Beside the times: the share of open ambient rays per setting, counted on the ray-query API
(svo_trace_rays -> svo_ambient_rays -> svo_trace_rays), which traces the same rays.

  python tools/ambient_bench.py [--rounds 12] [--block 40] [--settings off,N4_r8,reflect] [--bench-json LABEL=FILE ...]
                               [--out profiles/ambient_bench.json]

--bench-json: result lines of `python bench.py` runs to record beside the figures (the term off,
this tree and the parent commit's library alternated by the caller), as `label=path` pairs.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AMBIENT = (0.5, 0.75, 1.0)
INF = float("inf")
REFLECT = ((0.5, 0.25, 0.75), 7)
SETTINGS = [("off", 0, INF), ("N4_r8", 4, 8.0), ("N8_r8", 8, 8.0), ("N16_r8", 16, 8.0), ("N4_rinf", 4, INF),
            ("reflect", 0, INF)]


def open_shares(torch, rm, cam, w, h, mode):
    """Per setting: the primary hits, the ambient rays and the share of them that are open."""
    from raytracingtest_amd.query import camera_rays
    n = w * h
    c2w, inv_proj = cam.uniforms(w, h)
    d_rays = torch.from_numpy(camera_rays(c2w, inv_proj, w, h).view(np.uint8).reshape(-1).copy()).cuda()
    d_hits = torch.zeros(n * 6, dtype=torch.int32, device="cuda")
    d_vox = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rm.trace_rays_device(d_rays.data_ptr(), n, hits=d_hits.data_ptr(), voxel=d_vox.data_ptr(), stack_mode=mode, raw=True)
    rm.synchronize()
    primary = int((((d_hits.view(n, 6)[:, 1] >> 16) & 1) != 0).sum())
    out = {}
    for name, n_rays, radius in [s for s in SETTINGS if s[1]]:
        d_amb = torch.zeros(n * n_rays * 32, dtype=torch.uint8, device="cuda")
        d_hits2 = torch.zeros(n * n_rays * 6, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rm.ambient_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), d_vox.data_ptr(), d_amb.data_ptr(), n_rays, radius, 0,
                               raw=True)
        rm.trace_rays_device(d_amb.data_ptr(), n * n_rays, hits=d_hits2.data_ptr(), stack_mode=mode)
        rm.synchronize()
        flags = (d_hits2.view(n * n_rays, 6)[:, 1] >> 16) & 0xFFFF
        traced = int(((flags & 0x10) == 0).sum())
        is_open = int(((flags & 0x11) == 0).sum())
        out[name] = {"primary_hits": primary, "ambient_rays": traced, "open_share": round(is_open / max(traced, 1), 4)}
        del d_amb, d_hits2
    return out


def measure(torch, rm, cam, w, h, mode, args):
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
        for name, n_rays, radius in order:
            rm.SetAmbient(AMBIENT if n_rays else None, n_rays or 4, radius, 0)
            rm.SetReflection(*REFLECT) if name == "reflect" else rm.SetReflection(None)
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
    rm.SetAmbient(None)
    rm.SetReflection(None)
    rm.forget_stream(sptr)
    out = {}
    off = float(np.median(times["off"]))
    for name, n_rays, radius in SETTINGS:
        med = float(np.median(times[name]))
        out[name] = {"n_rays": n_rays, "radius": "inf" if radius == INF else radius, "frame_ms_median": round(med, 5),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ambient_bench.json"))
    args = ap.parse_args()
    if args.settings:
        keep = set(args.settings.split(",")) | {"off"}
        SETTINGS[:] = [s for s in SETTINGS if s[0] in keep]
    import torch
    from raytracingtest_amd import RaytracingMaster, build
    from raytracingtest_amd.camera import CAMERAS
    from raytracingtest_amd.native_builder import build_sampler_svo

    out = {"source_digest": build.source_digest(), "rounds": args.rounds, "block": args.block, "skip": args.skip,
           "ambient": list(AMBIENT), "variant": 0,
           "method": "events on the render's stream around each svo_render_device into an RGBA32F buffer (primary launch + "
                     "ambient pass); settings interleaved, first `skip` launches of each block dropped",
           "scenes": {}}
    w, h, mode = 1920, 1080, 0
    svo = build_sampler_svo(4, args.max_level)
    rm = RaytracingMaster(device=0, capacity_nodes=len(svo))
    rm.SetSVOBuffer(svo)
    for pose in ("flyover", "main"):
        print(f"== C3 depth {args.max_level - 1}, {len(svo)} nodes, {w}x{h}, {pose}", flush=True)
        cam = CAMERAS[pose]()
        scene = {"nodes": len(svo), "width": w, "height": h, "stack_mode": mode,
                 "settings": measure(torch, rm, cam, w, h, mode, args)}
        for name, share in open_shares(torch, rm, cam, w, h, mode).items():
            scene["settings"][name].update(share)
        print(json.dumps({"open": {k: v.get("open_share") for k, v in scene["settings"].items()}}), flush=True)
        out["scenes"][f"C3_{pose}"] = scene
    rm.close()
    runs = {}
    for item in args.bench_json:
        lab, path = item.split("=", 1)
        with open(path) as fh:
            lines = [ln for ln in fh if ln.lstrip().startswith("{")]
        runs.setdefault(lab, []).append(json.loads(lines[-1]))
    if runs:
        out["bench_py_ambient_off"] = runs
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
