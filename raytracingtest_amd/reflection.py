"""Specular bounce rays: the numpy statement of the bounce rule (csrc/svo_reflect.h,
svo_bounce_rays in include/svo_rt.h; INTEGRATION.md "Reflections").

From a ray as it was traced, origin o and direction d (a query's direction after its
small-direction clamp), and its hit record -- t (2048 x SVO t), normal n, hit_scale s, and the
integer coordinates c of the voxel key -- the bounce ray is, every operation one f32 rounding:

  1. box         side = 2^(s - 18), lo = c side - 16, hi = lo + side          (exact)
  2. entry face  face_k = d_k > 0 ? lo_k : hi_k, te_k = (face_k - o_k) (1 / d_k);
                 g = 0, then for k = 1, 2: g = k if te_k > te_g (a NaN never wins);
                 out = d_g > 0 ? -1 : +1
  3. origin      P = o + (t / 64) d for the axes k != g, face_g + out (side 2^-6) for g
  4. direction   dn = (n_0 d_0 + n_1 d_1) + n_2 d_2, r = d - (2 dn) n, and r_g = -r_g if r_g
                 points into the face; r is not renormalised (the reference does not either)
  5. the ray     {origin, t_max = +inf, r, reserved 0}

Deviation from the reference (documented): its Shade restarts the ray at P + 0.001 n
(RaytraceCompute.compute:97-104) with the smooth normal n, which on voxels very often lies on or
inside the voxel just hit.  Here the ray leaves through the cube face it entered by.
"""
import numpy as np

from ._lib import RAY_DTYPE
from .query import batch_arrays, sanitize_rays


def dead_rays(n):
    """n dead rays: all 32 bytes zero except t_max = +inf (a zero direction: invalid by the
    query's classify, so svo_trace_rays does not trace them)."""
    out = np.zeros(n, RAY_DTYPE)
    out["t_max"] = np.inf
    return out


def entry_face(o, d, hits, voxel):
    """Steps 1-3 of the rule on traced origins o and directions d ([n, 3] f32), their hit records and
    voxel keys: (g, out, org) = the entry axis [n], out = d_g > 0 ? -1 : +1 [n] and the origin [n, 3]
    of a ray that leaves through that face.  Shared with the ambient rule (ambient.py)."""
    f = np.float32
    rows = np.arange(len(o))
    with np.errstate(all="ignore"):
        side = np.ldexp(f(1.0), hits["hit_scale"].astype(np.int32) - 18).astype(f)[:, None]
        c = np.stack([(voxel >> np.uint64(21 * k)) & np.uint64(0x1FFFFF) for k in range(3)], axis=1).astype(f)
        lo = c * side - f(16.0)
        hi = lo + side
        face = np.where(d > 0, lo, hi)
        te = (face - o) * (f(1.0) / d)
        g = np.zeros(len(o), np.int64)
        for k in (1, 2):
            g = np.where(te[:, k] > te[rows, g], k, g)
        out = np.where(d[rows, g] > 0, f(-1.0), f(1.0)).astype(f)
        tw = hits["t"] * f(1.0 / 64.0)
        org = o + tw[:, None] * d
        org[rows, g] = face[rows, g] + out * (side[:, 0] * f(2.0 ** -6))
    return g, out, org


def bounce_rays(rays, hits, voxel, raw=False):
    """svo_bounce_rays in numpy: out[i] = the bounce ray of rays[i] (RAY_DTYPE) if hits[i]
    (HIT_DTYPE) has flag bit 0, else the dead ray.  voxel: the hits' voxel keys (uint64).
    raw: rays were traced with SVO_QUERY_RAW_DIRECTIONS (no small-direction clamp)."""
    f = np.float32
    rays, hits, voxel = batch_arrays(rays, hits, voxel)
    traced, _ = sanitize_rays(rays, raw=raw)
    o, d = traced["origin"], traced["dir"]
    n = np.stack([hits["nx"], hits["ny"], hits["nz"]], axis=1)
    rows = np.arange(len(rays))
    g, out, org = entry_face(o, d, hits, voxel)
    with np.errstate(all="ignore"):
        dn = n[:, 0] * d[:, 0]
        dn = dn + n[:, 1] * d[:, 1]
        dn = dn + n[:, 2] * d[:, 2]
        r = d - (f(2.0) * dn)[:, None] * n
        rg = r[rows, g]
        into = ((out > 0) & (rg < 0)) | ((out < 0) & (rg > 0))
        r[rows, g] = np.where(into, -rg, rg)
    res = dead_rays(len(rays))
    hit = (hits["flags"] & 1) != 0
    res["origin"][hit] = org[hit]
    res["dir"][hit] = r[hit]
    return res
