"""Shared helpers of the reflection tests (tests/test_reflection.py, tests/test_gpu_reflection.py): the
expected frame of a render with svo_set_reflection, built from the CPU oracle alone -- oracle.render_ex
for the primary rays, orc_camera_ray for their rays, orc_intersect_ex (with its albedo output) for every
bounce ray, reflection.bounce_rays for the rule, and the fold res += e * col in numpy f32.

A frame's paths do not depend on the specular setting (unless it is all zero), so the bounce generations
of a frame are traced once (generations) and folded per setting (expected_frame)."""
import ctypes
import functools

import numpy as np

from raytracingtest_amd import HIT_DTYPE
from raytracingtest_amd._lib import RAY_DTYPE
from raytracingtest_amd.camera import main_camera, main_light, overview_camera
from raytracingtest_amd.query import make_rays, sanitize_rays
from raytracingtest_amd.reflection import bounce_rays
from tests.guard_pools import diagonal_camera
from tests.split_cases import edge_camera

CAMS = {"main": main_camera, "overview": overview_camera}
# diagonal: the guarded pools' camera (tests/guard_pools.py); edge: the split tests' (tests/split_cases.py)
POSES = dict(CAMS, diagonal=diagonal_camera, edge=edge_camera)


def _geometry_camera(name):
    from tests import geometry_model
    return geometry_model.camera(name)


# geometry_<pool>: geometry_model.camera's view of one of its pools (tests/test_gpu_secondary_geometry.py)
POSES.update({f"geometry_{n}": functools.partial(_geometry_camera, n) for n in ("walk12", "walk16")})
SIZES = {"raster": (200, 120), "strips": (256, 128)}   # 25 tile columns: the raster path; 32: XCD strips
DEFAULT = ((0.5, 0.25, 0.75), 7)
SECOND = ((1.0, 0.0, 0.0), 2)
MAX_BOUNCES = 7

_cache = {}


def oracle_svo(oracle_mod, svo):
    return oracle_mod.OracleSVO(nodes=svo.to_v2(), attachments=svo.attachments)


def oracle_trace(oracle_mod, osvo, rays, mode=0):
    """orc_intersect_ex on every ray as given: (hits [n], albedo [n, 3], voxel keys [n])."""
    L = oracle_mod.lib()
    vp = ctypes.c_void_p
    L.orc_intersect_ex.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    L.orc_intersect_ex.restype = ctypes.c_int
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    n = len(rays)
    hits = np.zeros(n, HIT_DTYPE)
    alb = np.zeros((n, 3), np.float32)
    pos = np.zeros(4, np.float32)
    vox = np.zeros(n, np.uint64)
    base, o_off, d_off = rays.ctypes.data, RAY_DTYPE.fields["origin"][1], RAY_DTYPE.fields["dir"][1]
    svo_p, ph, pa, pv, pp = ctypes.addressof(osvo.s), hits.ctypes.data, alb.ctypes.data, vox.ctypes.data, pos.ctypes.data
    for i in range(n):
        L.orc_intersect_ex(svo_p, base + 32 * i + o_off, base + 32 * i + d_off, mode, ph + 24 * i, pa + 12 * i,
                           None, None, pp, pv + 8 * i)
    return hits, alb, vox


def primary(oracle_mod, name, svo, cam_name, w, h, mode=0, off=(0.5, 0.5)):
    """The reflection-off frame: oracle.render_ex's outputs, the indices of its hit pixels and their
    camera rays (orc_camera_ray) as a ray list."""
    key = ("primary", name, cam_name, w, h, mode, off)
    if key not in _cache:
        c2w, inv_proj = POSES[cam_name]().uniforms(w, h)
        ocam = oracle_mod.make_camera(c2w, inv_proj, off, main_light())
        hits, rgba, _, pos, vox = oracle_mod.render_ex(oracle_svo(oracle_mod, svo), ocam, w, h, mode)
        px = np.flatnonzero(hits["flags"] & 1)
        o = np.zeros((len(px), 3), np.float32)
        d = np.zeros((len(px), 3), np.float32)
        f, po, pd, cp = oracle_mod.lib().orc_camera_ray, o.ctypes.data, d.ctypes.data, ctypes.byref(ocam)
        for j, p in enumerate(px.tolist()):
            f(cp, p % w, p // w, w, h, po + 12 * j, pd + 12 * j)
        _cache[key] = {"hits": hits, "rgba": rgba.astype(np.float32), "position": pos, "voxel": vox, "px": px,
                       "rays": make_rays(o, d)}
    return _cache[key]


def generations(oracle_mod, name, svo, cam_name, w, h, mode=0, off=(0.5, 0.5)):
    """The frame's bounce generations 1 .. 7.  Generation b: `idx` the paths (indices into primary's px)
    that make a bounce ray, `src_rays` / `src_hits` / `src_voxel` / `raw` what it is made from, `rays` the
    bounce rays (reflection.bounce_rays), `traced` / `invalid` the query's front end on them, and for the
    valid ones (`idx[~invalid]`) `hits`, `albedo`, `voxel`: the oracle's trace."""
    key = ("generations", name, cam_name, w, h, mode, off)
    if key not in _cache:
        prim = primary(oracle_mod, name, svo, cam_name, w, h, mode, off)
        osvo = oracle_svo(oracle_mod, svo)
        idx = np.arange(len(prim["px"]))
        rays, hits, vox, raw = prim["rays"], prim["hits"][prim["px"]], prim["voxel"][prim["px"]], True
        gens = []
        for _ in range(MAX_BOUNCES):
            nxt = bounce_rays(rays, hits, vox, raw=raw)
            traced, invalid = sanitize_rays(nxt)
            h2, alb, v2 = oracle_trace(oracle_mod, osvo, traced[~invalid], mode)
            gens.append({"idx": idx, "src_rays": rays, "src_hits": hits, "src_voxel": vox, "raw": raw, "rays": nxt,
                         "traced": traced, "invalid": invalid, "hits": h2, "albedo": alb, "voxel": v2})
            go = (h2["flags"] & 1) != 0
            idx, rays, hits, vox, raw = idx[~invalid][go], nxt[~invalid][go], h2[go], v2[go], False
        _cache[key] = gens
    return _cache[key]


def shade_hit(normal, albedo, light):
    """Shade's hit branch in f32, as the kernels compute it: saturate(-dot(n, L)) * L.w * albedo."""
    f = np.float32
    L = np.asarray(light, f)
    with np.errstate(invalid="ignore"):
        d = normal[:, 0] * L[0]
        d = d + normal[:, 1] * L[1]
        d = d + normal[:, 2] * L[2]
        s = np.fmin(np.fmax(d * f(-1.0), f(0.0)), f(1.0)) * L[3]
        return (s[:, None] * albedo).astype(f)


def sky(dir_y):
    f = np.float32
    k = f(0.5) * dir_y.astype(f) + f(0.5)
    return np.stack([f(0.25) + f(0.5) * k, f(0.35) + f(0.55) * k, f(0.6) + f(0.4) * k], axis=1).astype(f)


def expected_frame(oracle_mod, name, svo, cam_name, w, h, mode=0, specular=DEFAULT[0], max_bounces=DEFAULT[1],
                   off=(0.5, 0.5)):
    """RGBA32F [w * h, 4] of the frame with svo_set_reflection(specular, max_bounces): per hit pixel
    res = the reflection-off colour, e = 1; per bounce e *= specular (all zero: stop), the bounce ray
    (invalid: stop), res += e * (shade of its hit | sky of its traced direction), a miss stops."""
    f = np.float32
    prim = primary(oracle_mod, name, svo, cam_name, w, h, mode, off)
    rgba = prim["rgba"].copy()
    spec = np.asarray(specular, f)
    if max_bounces == 0 or not spec.any():
        return rgba
    gens = generations(oracle_mod, name, svo, cam_name, w, h, mode, off)
    res = rgba[prim["px"], :3].copy()
    e = np.ones(3, f)
    for g in gens[:max_bounces]:
        e = e * spec
        if not e.any():
            break
        hit = (g["hits"]["flags"] & 1) != 0
        n = np.stack([g["hits"]["nx"], g["hits"]["ny"], g["hits"]["nz"]], axis=1)
        col = np.where(hit[:, None], shade_hit(n, g["albedo"], main_light()), sky(g["traced"]["dir"][~g["invalid"], 1]))
        at = g["idx"][~g["invalid"]]
        res[at] = res[at] + e[None, :] * col.astype(f)
    rgba[prim["px"], :3] = res
    return rgba


def path_lengths(gens, n_paths):
    """Per path the number of bounce rays it traces (valid ones)."""
    length = np.zeros(n_paths, np.int64)
    for g in gens:
        length[g["idx"][~g["invalid"]]] += 1
    return length
