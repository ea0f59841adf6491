"""Scene objects: the numpy statement of the object rule (csrc/svo_object.h, svo_set_objects / svo_trace_scene
/ svo_object_rays in include/svo_rt.h; INTEGRATION.md "Objects").

An object is a sub-SVO of the context's pool (its root's descriptor index) placed in the world: a cube of side
32 * 2^k world units centred at p and rotated by R (row-major, world = R * object).  For a world ray (o, d,
t_max), with s = 2^-k (exact), every operation one f32 rounding, only + - * /, compares and selects:

  1. classify the world ray as svo_trace_rays does (query.sanitize_rays): an invalid ray has no candidate
  2. q = o - p; o'_j = ((R_0j q_0 + R_1j q_1) + R_2j q_2) s; d'_j = ((R_0j d_0 + R_1j d_1) + R_2j d_2) s
     (object_rays).  Origin and direction take the same scale: the ray parameter is shared
  3. the object ray {o', t_max, d', 0} is classified again and, unless raw, clamped (query.sanitize_rays)
  4. cube test (cube_test): t_in / t_out = the walk's own entry (after max(.., 0)) and exit of the cube for the
     clamped object ray, t_entry = fl(fl(32 t_in) 64); walked iff t_in <= t_out and (the best record so far is
     a miss or t_entry < best.t)
  5. the walk from parent = root, the t (1 / 64) <= t_max filter (query.apply_t_max), the normal rotated to
     world (world_normal); position and voxel key stay object-local
  6. fold (fold_nearest): candidates in the order terrain, objects 0 .. n - 1; a later hit replaces the best
     iff the best is a miss or its t < the best t (strict: ties keep the earlier candidate)

(x 1 + y 0) + z 0 turns a -0 component into +0: an identity placement reproduces svo_trace_rays byte for byte
only on rays without negative-zero components.
"""
import numpy as np

from ._lib import HIT_DTYPE, MAX_OBJECTS, OBJECT_DTYPE, RAY_DTYPE
from .query import sanitize_rays
from .reflection import dead_rays

MAX_COORD = 2.0 ** 20
MAX_SCALE_LOG2 = 8
ORTHO_TOL = 2.0 ** -10
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def make_objects(objects):
    """OBJECT_DTYPE records of a list of (root, scale_log2, position, rotation[, flags[, reserved]]) tuples
    (rotation: 9 numbers row-major or a 3 x 3 array, None: the identity), or of OBJECT_DTYPE records as they
    are; checked as svo_set_objects checks them (the root's bound, the context's capacity, is the library's)."""
    if isinstance(objects, np.ndarray) and objects.dtype == OBJECT_DTYPE:
        out = np.ascontiguousarray(objects).reshape(-1).copy()
    else:
        objects = list(objects)
        out = np.zeros(len(objects), OBJECT_DTYPE)
        for j, ob in enumerate(objects):
            if isinstance(ob, np.void) and ob.dtype == OBJECT_DTYPE:   # a record among the tuples
                out[j] = ob
                continue
            if not 0 <= int(ob[0]) < 2 ** 32:
                raise ValueError("object root must be a descriptor index (uint32)")
            if not -2 ** 31 <= int(ob[1]) < 2 ** 31:
                raise ValueError("object scale_log2 must lie in [-8, 8]")
            out["root"][j] = int(ob[0])
            out["scale_log2"][j] = int(ob[1])
            out["position"][j] = ob[2]
            out["rotation"][j] = np.asarray(IDENTITY if ob[3] is None else ob[3], np.float32).reshape(9)
            out["flags"][j] = ob[4] if len(ob) > 4 else 0
            out["reserved"][j] = ob[5] if len(ob) > 5 else 0
    if len(out) > MAX_OBJECTS:
        raise ValueError(f"{len(out)} objects, at most {MAX_OBJECTS}")
    if (np.abs(out["scale_log2"].astype(np.int64)) > MAX_SCALE_LOG2).any():
        raise ValueError("object scale_log2 must lie in [-8, 8]")
    if out["flags"].any():
        raise ValueError("unknown object flag bits")
    if out["reserved"].any():
        raise ValueError("object reserved word must be 0")
    with np.errstate(invalid="ignore"):
        if not (np.abs(out["position"]) <= MAX_COORD).all():
            raise ValueError("object position components must be finite and lie in [-2^20, 2^20]")
    R = out["rotation"].astype(np.float64).reshape(-1, 3, 3)
    if not np.isfinite(R).all():
        raise ValueError("object rotation entries must be finite")
    err = R @ R.transpose(0, 2, 1) - np.eye(3)
    if not (np.abs(err) <= ORTHO_TOL).all():
        raise ValueError("object rotation must be orthonormal (R R^T - I within 2^-10)")
    if len(R) and not (np.linalg.det(R) > 0).all():
        raise ValueError("object rotation must have a positive determinant")
    return out


def _one(obj):
    """One object: an OBJECT_DTYPE record, a one-element array or list, or one make_objects tuple."""
    if isinstance(obj, np.void) and obj.dtype == OBJECT_DTYPE:
        return obj
    if isinstance(obj, tuple) and len(obj) >= 4 and np.ndim(obj[0]) == 0 and not isinstance(obj[0], np.void):
        obj = [obj]
    obj = make_objects(obj)
    if isinstance(obj, np.ndarray):
        if len(obj) != 1:
            raise ValueError(f"one object expected, {len(obj)} given")
        obj = obj[0]
    return obj


def object_rays(rays, obj):
    """svo_object_rays in numpy: out[i] = rays[i] (RAY_DTYPE) in the object's frame BEFORE the clamp, {o', t_max,
    d', 0}; the dead ray (reflection.dead_rays) where the world ray is invalid."""
    f = np.float32
    rays = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1)
    obj = _one(obj)
    _, invalid = sanitize_rays(rays, raw=True)
    s = f(2.0) ** f(-int(obj["scale_log2"]))
    R = obj["rotation"].astype(f)
    p = obj["position"].astype(f)
    out = dead_rays(len(rays))
    with np.errstate(all="ignore"):
        q = (rays["origin"] - p[None, :]).astype(f)
        d = rays["dir"]
        for j in range(3):
            a = R[j] * q[:, 0]
            a = a + R[3 + j] * q[:, 1]
            a = a + R[6 + j] * q[:, 2]
            b = R[j] * d[:, 0]
            b = b + R[3 + j] * d[:, 1]
            b = b + R[6 + j] * d[:, 2]
            out["origin"][:, j] = np.where(invalid, f(0.0), (a * s).astype(f))
            out["dir"][:, j] = np.where(invalid, f(0.0), (b * s).astype(f))
    out["t_max"] = np.where(invalid, f(np.inf), rays["t_max"])
    return out


def _sel_max(a, b):
    return np.where((a > b) | np.isnan(b), a, b)


def _sel_min(a, b):
    return np.where((a < b) | np.isnan(b), a, b)


def cube_span(rays):
    """(t_in, t_out) [n] f32: the walk's own entry (after its max(.., 0)) and exit of the cube for the object
    rays AS TRACED (after the clamp): svo_kernel.hip setup_ray's t_min and t_max."""
    f = np.float32
    rays = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1)
    with np.errstate(all="ignore"):
        x = rays["origin"] * f(1.0 / 32.0) + f(1.5)
        d = rays["dir"]
        coef = f(1.0) / -np.abs(d)
        bias = coef * x
        bias = np.where(d > 0, f(3.0) * coef - bias, bias).astype(f)
        lo = (f(2.0) * coef - bias).astype(f)
        hi = (coef - bias).astype(f)
        t_min = _sel_max(_sel_max(lo[:, 0], lo[:, 1]), lo[:, 2])
        t_out = _sel_min(_sel_min(hi[:, 0], hi[:, 1]), hi[:, 2])
        t_in = np.where(t_min > 0, t_min, f(0.0))
    return t_in.astype(f), t_out.astype(f)


def entry_t(t_in):
    """t_entry = fl(fl(32 t_in) 64): the cube entry in a record's t units."""
    f = np.float32
    with np.errstate(all="ignore"):
        return ((np.asarray(t_in, f) * f(32.0)).astype(f) * f(64.0)).astype(f)


def cube_test(rays, best_hit=None, best_t=None):
    """Step 4 for the object rays AS TRACED: the mask of the rays that walk the object.  best_hit [n] bool,
    best_t [n] f32: flag bit 0 and t of the best record so far (None: every best is a miss)."""
    t_in, t_out = cube_span(rays)
    with np.errstate(invalid="ignore"):
        go = t_in <= t_out
        if best_hit is not None:
            go &= ~np.asarray(best_hit, bool) | (entry_t(t_in) < np.asarray(best_t, np.float32))
    return go


def world_normal(hits, obj):
    """The records with their normals rotated to world, n_i = (R_i0 m_0 + R_i1 m_1) + R_i2 m_2 (not
    renormalised); records without flag bit 0 stay as they are."""
    f = np.float32
    hits = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1).copy()
    R = _one(obj)["rotation"].astype(f)
    hit = (hits["flags"] & 1) != 0
    m = [hits["nx"].copy(), hits["ny"].copy(), hits["nz"].copy()]
    with np.errstate(all="ignore"):
        for i, name in enumerate(("nx", "ny", "nz")):
            a = R[3 * i] * m[0]
            a = a + R[3 * i + 1] * m[1]
            a = a + R[3 * i + 2] * m[2]
            hits[name] = np.where(hit, a.astype(f), hits[name])
    return hits


def fold_nearest(best, best_id, cand, cand_id, walked=None):
    """Step 6 for one more candidate: best, cand HIT_DTYPE [n]; best_id int32 [n]; cand_id the candidate's
    object id (0 terrain, j + 1 object j); walked [n] bool: the rays for which the candidate exists at all
    (the cube test's mask; None: all).  Returns (taken, best, best_id): taken [n] bool, the rays whose best is
    now the candidate."""
    best = np.ascontiguousarray(best, HIT_DTYPE).reshape(-1).copy()
    cand = np.ascontiguousarray(cand, HIT_DTYPE).reshape(-1)
    best_id = np.asarray(best_id, np.int32).copy()
    best_hit = (best["flags"] & 1) != 0
    cand_hit = (cand["flags"] & 1) != 0
    if walked is not None:
        cand_hit &= np.asarray(walked, bool)
    with np.errstate(invalid="ignore"):
        taken = cand_hit & (~best_hit | (cand["t"] < best["t"]))
    best[taken] = cand[taken]
    best_id[taken] = cand_id
    return taken, best, best_id
