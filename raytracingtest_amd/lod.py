"""Level-of-detail helpers (svo_set_lod / svo_trace_rays_lod, include/svo_rt.h)."""
import numpy as np


def pixel_footprint(inv_proj, height, pixels=1.0):
    """ray_size_coef for a camera: the footprint of `pixels` pixels at the frame's centre per unit t
    of a unit-length ray, pixels * 2 * |inv_proj[1][1]| / height (inv_proj: the 4x4 inverse
    projection as UpdateShaderParameters takes it, row-major indexing)."""
    return float(pixels) * 2.0 * abs(float(np.asarray(inv_proj)[1][1])) / float(height)


def lod_hit_is_inner(svo, hits):
    """Per hit record (HIT_DTYPE or COMPACT_DTYPE array): True where the hit voxel is an inner one,
    i.e. the pool's non-leaf bit of (parent, hit_idx) is set -- a level-of-detail hit.  Misses: False."""
    hits = np.asarray(hits)
    parent = hits["parent"].astype(np.int64)
    if "hit_idx" in hits.dtype.names:
        idx, hit = hits["hit_idx"].astype(np.uint32), (hits["flags"] & 1) != 0
    else:
        idx, hit = hits["meta"] & 0xFF, ((hits["meta"] >> 16) & 1) != 0
    lo, _ = svo.masks_and_first()
    safe = np.where(hit & (parent < len(lo)), parent, 0)
    return hit & (((lo[safe] >> idx.astype(np.uint32)) & 1) != 0)
