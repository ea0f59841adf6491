#!/usr/bin/env python3
"""The skybox on the bench's C3 scene (depth-11 Custom1 terrain, 1920x1080): what the sky pass costs a
frame, at the flyover and the overview pose, for the settings no texture, a 2048x1024 texture sampled
nearest, and the same texture sampled bilinear.

Timing: the whole render of a frame into an RGBA32F device buffer -- the primary launch plus, with a
texture set, the sky pass -- bracketed by events on the render's stream.  The settings are interleaved
in one process: ROUNDS rounds, each visiting every setting once for BLOCK launches at a held view, of
which the first SKIP are dropped.  Reported: the median over all kept launches of a setting, the spread
of the per-round medians (min, max), the cost against the same run's no-texture frame, and the frame's
miss pixels.  Not pass/fail numbers.

  python tools/sky_bench.py [--rounds 12] [--block 40] [--bench-json LABEL=FILE ...] [--out profiles/sky_bench.json]

--bench-json: result lines of `python bench.py` runs to record beside the figures (no texture, this
tree and the parent commit's library alternated by the caller), as `label=path` pairs.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEX_W, TEX_H = 2048, 1024
SETTINGS = [("none", None), ("nearest", False), ("bilinear", True)]


def panorama():
    """A 2048x1024 RGBA32F panorama: a vertical gradient with per-texel noise (the values do not matter to
    the timing; the addresses do)."""
    rng = np.random.default_rng(1)
    v = np.linspace(0.0, 1.0, TEX_H, dtype=np.float32)[:, None, None]
    t = np.empty((TEX_H, TEX_W, 4), np.float32)
    t[:, :, :3] = 0.2 + 0.6 * v + 0.2 * rng.random((TEX_H, TEX_W, 3), dtype=np.float32)
    t[:, :, 3] = 1.0
    return t


def miss_pixels(torch, rm, w, h, mode):
    n_tiles = ((w + 7) // 8) * ((h + 7) // 8)
    masks = torch.zeros(n_tiles, dtype=torch.int64, device="cuda")
    rgba8 = torch.zeros(w * h, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rm.render_frame(w, h, stack_mode=mode, rgba8=rgba8.data_ptr(), hitmask=masks.data_ptr())
    rm.synchronize()
    bits = np.unpackbits(masks.cpu().numpy().view(np.uint8))
    return w * h - int(bits.sum())


def measure(torch, rm, tex, cam, w, h, mode, args):
    n = w * h
    stream = torch.cuda.Stream()
    sptr = stream.cuda_stream
    d_rgba = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rm.UpdateShaderParameters(cam, w, h)
    times = {name: [] for name, _ in SETTINGS}
    rounds = {name: [] for name, _ in SETTINGS}
    for r in range(args.rounds + 1):           # round 0: warm-up of every setting's kernels
        order = SETTINGS if r % 2 == 0 else SETTINGS[::-1]
        for name, bilinear in order:
            if bilinear is None:
                rm.SetSkybox(None)
            else:
                rm.SetSkybox(tex, bilinear=bilinear)
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
    rm.SetSkybox(None)
    rm.forget_stream(sptr)
    out = {}
    off = float(np.median(times["none"]))
    for name, _ in SETTINGS:
        med = float(np.median(times[name]))
        out[name] = {"frame_ms_median": round(med, 5),
                     "frame_ms_round_medians_min_max": [round(min(rounds[name]), 5), round(max(rounds[name]), 5)],
                     "launches_timed": len(times[name]), "ms_over_no_texture": round(med - off, 5),
                     "multiple_of_no_texture_frame": round(med / off, 4)}
        print(json.dumps({name: out[name]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--skip", type=int, default=10)
    ap.add_argument("--max-level", type=int, default=11)
    ap.add_argument("--bench-json", action="append", default=[], metavar="LABEL=FILE")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sky_bench.json"))
    args = ap.parse_args()
    import torch
    from raytracingtest_amd import RaytracingMaster, build
    from raytracingtest_amd.camera import CAMERAS
    from raytracingtest_amd.native_builder import build_sampler_svo

    out = {"source_digest": build.source_digest(), "rounds": args.rounds, "block": args.block, "skip": args.skip,
           "texture": [TEX_W, TEX_H],
           "method": "events on the render's stream around each svo_render_device into an RGBA32F buffer (primary launch + "
                     "sky pass); settings interleaved, first `skip` launches of each block dropped",
           "scenes": {}}
    w, h, mode = 1920, 1080, 0
    tex = panorama()
    svo = build_sampler_svo(4, args.max_level)
    rm = RaytracingMaster(device=0, capacity_nodes=len(svo))
    rm.SetSVOBuffer(svo)
    for pose in ("flyover", "overview"):
        print(f"== C3 depth {args.max_level - 1}, {len(svo)} nodes, {w}x{h}, {pose}", flush=True)
        cam = CAMERAS[pose]()
        rm.UpdateShaderParameters(cam, w, h)
        scene = {"nodes": len(svo), "width": w, "height": h, "stack_mode": mode,
                 "miss_pixels": miss_pixels(torch, rm, w, h, mode),
                 "settings": measure(torch, rm, tex, cam, w, h, mode, args)}
        print(json.dumps({"miss_pixels": scene["miss_pixels"]}), flush=True)
        out["scenes"][f"C3_{pose}"] = scene
    rm.close()
    runs = {}
    for item in args.bench_json:
        lab, path = item.split("=", 1)
        with open(path) as fh:
            lines = [ln for ln in fh if ln.lstrip().startswith("{")]
        runs.setdefault(lab, []).append(json.loads(lines[-1]))
    if runs:
        out["bench_py_no_texture"] = runs
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
