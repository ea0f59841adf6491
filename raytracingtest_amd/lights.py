"""Point lights: the numpy statement of the light rule (csrc/svo_light.h, svo_set_lights / svo_light_rays in
include/svo_rt.h; INTEGRATION.md "Lights").

From a ray as it was traced (origin o, direction d after the query's clamp), its hit record (t, hit_scale,
the voxel key, the normal n) and a light (position p, range R, colour c, flags), every operation one f32
rounding, only + - * /, sqrt, compares and selects:

  1. steps 1-3 of the bounce rule (reflection.entry_face): the entry axis g, out = d_g > 0 ? -1 : +1, the
     origin Q (P off the axis g, face_g + out (side 2^-6) on it)
  2. L_k = p_k - Q_k; facing iff L_g out > 0                                   (ordered; the product is exact)
  3. d2 = (L0 L0 + L1 L1) + L2 L2, u = d2 / (R R); in range iff u < 1          (ordered; NaN: false)
  4. not facing, or out of range: no ray and no contribution
  5. the shadow ray {Q, t_max = 1, dir = L, reserved 0}, traced as svo_trace_rays traces it with flags 0
     (classify, the small-direction clamp -- shading keeps L --, the walk, then t (1 / 64) <= t_max on the
     finished record).  Lit iff the record has neither flag bit 0 nor bit 4; LIGHT_NO_SHADOW skips the step
  6. dist = sqrt(d2); ndl = ((n0 L0 + n1 L1) + n2 L2) / dist; s = ndl > 0 ? ndl : 0, then s < 1 ? s : 1;
     w = 1 - u u, w = w w; a = w / (1 + d2); k = s a; contrib_c = (k c_c) alb_c
  7. per hit pixel res = the lights-off colour; for j in order, if lit by j: res_c = res_c + contrib_c
"""
import numpy as np

from ._lib import LIGHT_DTYPE, LIGHT_NO_SHADOW, MAX_LIGHTS
from .query import batch_arrays, sanitize_rays
from .reflection import dead_rays, entry_face

MAX_COORD = 2.0 ** 20
MAX_COLOUR = 65536.0


def make_lights(lights):
    """LIGHT_DTYPE records of a list of (position, range, colour[, flags]) tuples, or of LIGHT_DTYPE records
    as they are; checked as svo_set_lights checks them."""
    if isinstance(lights, np.ndarray) and lights.dtype == LIGHT_DTYPE:
        out = np.ascontiguousarray(lights).reshape(-1).copy()
    else:
        lights = list(lights)
        out = np.zeros(len(lights), LIGHT_DTYPE)
        for j, l in enumerate(lights):
            out["position"][j] = l[0]
            out["range"][j] = l[1]
            out["colour"][j] = l[2]
            out["flags"][j] = l[3] if len(l) > 3 else 0
    if len(out) > MAX_LIGHTS:
        raise ValueError(f"{len(out)} lights, at most {MAX_LIGHTS}")
    with np.errstate(invalid="ignore"):
        if not (np.abs(out["position"]) <= MAX_COORD).all():
            raise ValueError("light position components must be finite and lie in [-2^20, 2^20]")
        if not ((out["range"] > 0) & (out["range"] <= MAX_COORD)).all():
            raise ValueError("light range must lie in (0, 2^20]")
        if not ((out["colour"] >= 0) & (out["colour"] <= MAX_COLOUR)).all():
            raise ValueError("light colour components must lie in [0, 65536]")
    if (out["flags"] & ~np.uint32(LIGHT_NO_SHADOW)).any():
        raise ValueError("unknown light flag bits")
    return out


def _geometry(rays, hits, voxel, lights, raw):
    """Steps 1-3 for every (record, light) pair: hit [n], Q [n, 3], L [n, m, 3], d2, u, facing, in_range [n, m]."""
    f = np.float32
    rays, hits, voxel = batch_arrays(rays, hits, voxel)
    lights = make_lights(lights)
    n = len(rays)
    rows = np.arange(n)
    traced, _ = sanitize_rays(rays, raw=raw)
    g, out, Q = entry_face(traced["origin"], traced["dir"], hits, voxel)
    with np.errstate(all="ignore"):
        L = (lights["position"][None, :, :] - Q[:, None, :]).astype(f)
        L_g = L[rows, :, g]
        facing = L_g * out[:, None] > 0
        d2 = L[:, :, 0] * L[:, :, 0]
        d2 = d2 + L[:, :, 1] * L[:, :, 1]
        d2 = d2 + L[:, :, 2] * L[:, :, 2]
        R = lights["range"][None, :]
        u = (d2 / (R * R)).astype(f)
        in_range = u < 1
    hit = (hits["flags"] & 1) != 0
    return hit, hits, lights, Q, L, d2.astype(f), u, facing & hit[:, None], in_range & hit[:, None]


def light_rays(rays, hits, voxel, lights, raw=False):
    """svo_light_rays in numpy: out[i * n_lights + j] = the shadow ray of rays[i] (RAY_DTYPE) toward lights[j]
    if hits[i] (HIT_DTYPE) has flag bit 0 and the light is facing and in range, else the dead ray.  voxel: the
    hits' voxel keys (uint64).  raw: rays were traced with SVO_QUERY_RAW_DIRECTIONS.  The lights' flags are
    not read."""
    hit, hits, lights, Q, L, d2, u, facing, in_range = _geometry(rays, hits, voxel, lights, raw)
    n, m = len(hits), len(lights)
    res = dead_rays(n * m).reshape(n, m)
    go = facing & in_range
    res["origin"][go] = np.broadcast_to(Q[:, None, :], (n, m, 3))[go]
    res["dir"][go] = L[go]
    res["t_max"][go] = np.float32(1.0)
    return res.reshape(-1)


def light_terms(rays, hits, voxel, lights, raw=False):
    """Per (record, light): (facing [n, m] bool, in_range [n, m] bool, k [n, m] f32), k the factor of step 6.
    Without flag bit 0 both flags are False; k is 0 unless the light is facing and in range."""
    f = np.float32
    hit, hits, lights, Q, L, d2, u, facing, in_range = _geometry(rays, hits, voxel, lights, raw)
    nrm = np.stack([hits["nx"], hits["ny"], hits["nz"]], axis=1)[:, None, :]
    with np.errstate(all="ignore"):
        dist = np.sqrt(d2)
        dot = nrm[:, :, 0] * L[:, :, 0]
        dot = dot + nrm[:, :, 1] * L[:, :, 1]
        dot = dot + nrm[:, :, 2] * L[:, :, 2]
        ndl = dot / dist
        s = np.where(ndl > 0, ndl, f(0.0)).astype(f)
        s = np.where(s < 1, s, f(1.0)).astype(f)
        w = f(1.0) - u * u
        w = w * w
        a = w / (f(1.0) + d2)
        k = (s * a).astype(f)
    k = np.where(facing & in_range, k, f(0.0)).astype(f)
    return facing, in_range, k


def fold(res, lit, k, lights, albedo):
    """Step 7 on res [n, 3] f32 (the lights-off colours): lit [n, m] bool, k [n, m] f32 (light_terms), albedo
    [n, 3] f32.  Returns the new colours; the sum runs in light order."""
    f = np.float32
    lights = make_lights(lights)
    res = np.asarray(res, f).copy()
    albedo = np.asarray(albedo, f)
    for j in range(len(lights)):
        contrib = ((k[:, j, None] * lights["colour"][j][None, :]).astype(f) * albedo).astype(f)
        res = np.where(lit[:, j, None], res + contrib, res).astype(f)
    return res
