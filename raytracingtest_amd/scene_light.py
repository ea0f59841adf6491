"""Objects in light: the numpy statement of the scene-light rule (csrc/svo_scene_light.h, svo_scene_light_rays
in include/svo_rt.h; INTEGRATION.md "Objects in light"): the light rule (lights.py) for the records of a scene
query (svo_trace_scene), whose hit may lie on a placed object, a rotated and scaled voxel.

Every operation is one f32 rounding, only + - * /, sqrt, compares and selects.

(a) Origin and face of a scene hit, from the traced world ray (o, d) AS GIVEN, the record (t, hit_scale, the
    world normal n), the voxel key and the object id (-1 a miss, 0 the terrain, c + 1 object c):
      - id -1, an id outside -1 .. n_objects, or a record without flag bit 0: nothing, every light gets the
        dead ray
      - id 0: the light rule unchanged (the clamp on d unless raw, reflection.entry_face: g, out, Q);
        N = out e_g
      - id c + 1, objects[c] = (k, p, R):
          1. (o', d') = step 2 of the object rule from the world ray as given, then the small-direction clamp
             on d' unless raw
          2. (g, out, Q') = reflection.entry_face(o', d', t, hit_scale, key)
          3. Q_i = (((R_i0 Q'_0 + R_i1 Q'_1) + R_i2 Q'_2) 2^k) + p_i;  N_i = out R_ig  (exact)
(b) Toward a light (p_l, range, colour): L = p_l - Q; an object hit is facing iff
    (N_0 L_0 + N_1 L_1) + N_2 L_2 > 0, the terrain keeps L_g out > 0; d2, u and "in range" are the light
    rule's.  Not facing or out of range: the dead ray; otherwise {Q, t_max 1, L, 0}, and the factor is the
    light rule's k with the record's world normal.
"""
import numpy as np

from ._lib import HIT_DTYPE
from .lights import make_lights
from .objects import make_objects
from .query import DIR_EPSILON, batch_arrays
from .reflection import dead_rays, entry_face


def _clamp(d, raw):
    """The small-direction clamp of the ray queries on directions [n, 3] (a copy; unchanged with raw)."""
    d = np.array(d, np.float32)
    if not raw:
        with np.errstate(invalid="ignore"):
            small = np.abs(d) < DIR_EPSILON
        d[small] = np.copysign(DIR_EPSILON, d[small])
    return d


def object_frame(o, d, obj):
    """Step 2 of the object rule on origins o and directions d [n, 3], with no classification: (o', d')."""
    f = np.float32
    s = f(2.0) ** f(-int(obj["scale_log2"]))
    R = obj["rotation"].astype(f)
    p = obj["position"].astype(f)
    o2 = np.zeros_like(o)
    d2 = np.zeros_like(d)
    with np.errstate(all="ignore"):
        q = (o - p[None, :]).astype(f)
        for j in range(3):
            a = R[j] * q[:, 0]
            a = a + R[3 + j] * q[:, 1]
            a = a + R[6 + j] * q[:, 2]
            b = R[j] * d[:, 0]
            b = b + R[3 + j] * d[:, 1]
            b = b + R[6 + j] * d[:, 2]
            o2[:, j] = a * s
            d2[:, j] = b * s
    return o2, d2


def scene_faces(rays, hits, voxel, object_id, objects, raw=False):
    """(a) for every record: (live [n] bool, terrain [n] bool, g [n], out [n] f32, Q [n, 3] f32, N [n, 3] f32,
    Qp [n, 3] f32).  live: flag bit 0 and an id in 0 .. n_objects; the other rows hold zeros.  Qp: the origin in
    the hit's own frame (Q' of step 2; Q itself for the terrain)."""
    f = np.float32
    rays, hits, voxel = batch_arrays(rays, hits, voxel)
    objects = make_objects(objects if objects is not None else [])
    ids = np.ascontiguousarray(object_id, np.int32).reshape(-1)
    n = len(rays)
    if len(ids) != n:
        raise ValueError(f"{n} rays, {len(ids)} object ids")
    live = ((hits["flags"] & 1) != 0) & (ids >= 0) & (ids <= len(objects))
    g = np.zeros(n, np.int64)
    out = np.zeros(n, f)
    Q = np.zeros((n, 3), f)
    N = np.zeros((n, 3), f)
    Qp = np.zeros((n, 3), f)
    o, d = rays["origin"], rays["dir"]
    at = np.flatnonzero(live & (ids == 0))
    if len(at):
        g[at], out[at], Q[at] = entry_face(o[at], _clamp(d[at], raw), hits[at], voxel[at])
        N[at, g[at]] = out[at]
        Qp[at] = Q[at]
    for c, ob in enumerate(objects):
        at = np.flatnonzero(live & (ids == c + 1))
        if not len(at):
            continue
        o2, d2 = object_frame(o[at], d[at], ob)
        gg, oo, qp = entry_face(o2, _clamp(d2, raw), hits[at], voxel[at])
        R = ob["rotation"].astype(f).reshape(3, 3)
        s = f(2.0) ** f(int(ob["scale_log2"]))
        with np.errstate(all="ignore"):
            for i in range(3):
                a = R[i, 0] * qp[:, 0]
                a = a + R[i, 1] * qp[:, 1]
                a = a + R[i, 2] * qp[:, 2]
                Q[at, i] = a * s + ob["position"][i]
                N[at, i] = oo * R[i, gg]
        g[at], out[at], Qp[at] = gg, oo, qp
    return live, live & (ids == 0), g, out, Q, N, Qp


def _geometry(rays, hits, voxel, object_id, objects, lights, raw):
    f = np.float32
    lights = make_lights(lights)
    live, terrain, g, out, Q, N, _ = scene_faces(rays, hits, voxel, object_id, objects, raw)
    rows = np.arange(len(Q))
    with np.errstate(all="ignore"):
        L = (lights["position"][None, :, :] - Q[:, None, :]).astype(f)
        facing_axis = L[rows, :, g] * out[:, None] > 0
        s = N[:, None, 0] * L[:, :, 0]
        s = s + N[:, None, 1] * L[:, :, 1]
        s = s + N[:, None, 2] * L[:, :, 2]
        facing = np.where(terrain[:, None], facing_axis, s > 0)
        d2 = L[:, :, 0] * L[:, :, 0]
        d2 = d2 + L[:, :, 1] * L[:, :, 1]
        d2 = d2 + L[:, :, 2] * L[:, :, 2]
        R = lights["range"][None, :]
        u = (d2 / (R * R)).astype(f)
        in_range = u < 1
    return lights, live, Q, L, d2.astype(f), u, facing & live[:, None], in_range & live[:, None]


def scene_light_rays(rays, hits, voxel, object_id, objects, lights, raw=False):
    """svo_scene_light_rays in numpy: out[i * n_lights + j] = the world-space shadow ray of rays[i] (RAY_DTYPE,
    as given to svo_trace_scene) toward lights[j] if hits[i] (HIT_DTYPE) has flag bit 0, object_id[i] lies in
    0 .. n_objects and the light is facing and in range, else the dead ray.  voxel: the hits' voxel keys
    (uint64, object-local); raw: rays were traced with SVO_QUERY_RAW_DIRECTIONS.  The lights' flags and the
    objects' roots are not read."""
    lights, live, Q, L, d2, u, facing, in_range = _geometry(rays, hits, voxel, object_id, objects, lights, raw)
    n, m = len(Q), len(lights)
    res = dead_rays(n * m).reshape(n, m)
    go = facing & in_range
    res["origin"][go] = np.broadcast_to(Q[:, None, :], (n, m, 3))[go]
    res["dir"][go] = L[go]
    res["t_max"][go] = np.float32(1.0)
    return res.reshape(-1)


def scene_light_terms(rays, hits, voxel, object_id, objects, lights, raw=False):
    """Per (record, light): (facing [n, m] bool, in_range [n, m] bool, k [n, m] f32), k the light rule's factor
    with the record's world normal.  Both flags are False for a record that is not live; k is 0 unless the
    light is facing and in range."""
    f = np.float32
    lights, live, Q, L, d2, u, facing, in_range = _geometry(rays, hits, voxel, object_id, objects, lights, raw)
    hits = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
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

