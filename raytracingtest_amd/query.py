"""Ray queries: caller-supplied ray batches for svo_trace_rays (include/svo_rt.h).

make_rays packs origins and directions into svo_ray records; sanitize_rays is the
numpy mirror of the library's classify-then-clamp rule, so a caller (or a test)
knows exactly which rays were traced and with which directions:

  1. classify: a ray is invalid if any origin or direction component is
     non-finite, if t_max is NaN, or if all three direction components are zero;
  2. clamp: unless raw, every direction component with |d| < 2^-23 becomes
     copysign(2^-23, d) -- Laine-Karras's small-direction clamp, which the
     reference commented out (NVIDIASVO.compute:21-24); without it an exactly
     axis-aligned ray misses everything.
"""
import numpy as np

from ._lib import HIT_DTYPE, RAY_DTYPE

DIR_EPSILON = np.float32(2.0 ** -23)   # exp2(-s_max), NVIDIASVO.compute:2-3


def make_rays(origins, dirs, t_max=np.inf):
    """svo_ray records (RAY_DTYPE) of n rays: origins, dirs [n, 3] world space (a
    direction is used as given, not normalised), t_max a scalar or [n] (+inf: no
    limit; a hit at record t stays a hit iff t / 64 <= t_max)."""
    origins = np.asarray(origins, np.float32).reshape(-1, 3)
    dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
    if len(origins) != len(dirs):
        raise ValueError(f"{len(origins)} origins for {len(dirs)} directions")
    rays = np.zeros(len(origins), RAY_DTYPE)
    rays["origin"] = origins
    rays["dir"] = dirs
    rays["t_max"] = np.broadcast_to(np.asarray(t_max, np.float32), (len(rays),))
    return rays


def batch_arrays(rays, hits, voxel):
    """A traced batch as the bounce, ambient and light-ray calls take it: (rays, hits, voxel) contiguous and
    flat, RAY_DTYPE, HIT_DTYPE and uint64, one hit record and one voxel key per ray."""
    rays = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1)
    hits = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    voxel = np.ascontiguousarray(voxel, np.uint64).reshape(-1)
    if not len(rays) == len(hits) == len(voxel):
        raise ValueError(f"{len(rays)} rays, {len(hits)} hit records, {len(voxel)} voxel keys")
    return rays, hits, voxel


def sanitize_rays(rays, raw=False):
    """(rays_as_traced, invalid_mask): what svo_trace_rays does to each ray before
    it traces it.  invalid_mask[i]: ray i is not traced (it gets the miss record
    with flag 0x10).  rays_as_traced: a copy with the clamped directions
    (unchanged with raw=True, SVO_QUERY_RAW_DIRECTIONS)."""
    rays = np.asarray(rays, RAY_DTYPE)
    out = rays.copy()
    d = out["dir"]
    invalid = ~(np.isfinite(rays["origin"]).all(axis=-1) & np.isfinite(d).all(axis=-1))
    invalid |= np.isnan(rays["t_max"])
    invalid |= (d == 0).all(axis=-1)
    if not raw:
        with np.errstate(invalid="ignore"):
            small = np.abs(d) < DIR_EPSILON
        d[small] = np.copysign(DIR_EPSILON, d[small])
    return out, invalid


def camera_rays(c2w, inv_proj, width, height, pixel_offset=(0.5, 0.5)):
    """The primary rays of a width x height frame as a ray list in raster order (index
    y * width + x): CreateCameraRay (RaytraceCompute.compute:129-151) in f32, operation by
    operation as the render kernel computes it, so a query of this list with raw=True
    gives the frame's own hit records.  c2w, inv_proj: 4x4 in mathematical (row, column)
    order (Camera.uniforms)."""
    f = np.float32
    c2w = np.asarray(c2w, f)
    inv = np.asarray(inv_proj, f)
    x = np.arange(width, dtype=f)[None, :].repeat(height, 0).reshape(-1)
    y = np.arange(height, dtype=f)[:, None].repeat(width, 1).reshape(-1)
    u = (x + f(pixel_offset[0])) / f(width) * f(2.0) - f(1.0)
    v = (y + f(pixel_offset[1])) / f(height) * f(2.0) - f(1.0)

    def mul4(m, v0, v1, v2, v3):   # HLSL mul(M, v) summed left to right, rows 0..2
        return [((m[r, 0] * v0 + m[r, 1] * v1) + m[r, 2] * v2) + m[r, 3] * v3 for r in range(3)]

    zero, one = f(0.0), f(1.0)
    org = mul4(c2w, zero, zero, zero, one)
    pd = mul4(inv, u, v, zero, one)
    d = mul4(c2w, pd[0], pd[1], pd[2], zero)
    inv_len = one / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    dirs = np.stack([d[0] * inv_len, d[1] * inv_len, d[2] * inv_len], axis=1).astype(f)
    return make_rays(np.broadcast_to(np.asarray(org, f), (width * height, 3)), dirs)


def apply_t_max(hits, t_max):
    """Mask of the hit records that svo_trace_rays' t_max filter keeps:
    flag bit 0 set and t * (1 / 64) <= t_max in f32."""
    with np.errstate(invalid="ignore"):
        return ((hits["flags"] & 1) != 0) & (hits["t"] * np.float32(1.0 / 64.0) <= np.asarray(t_max, np.float32))
