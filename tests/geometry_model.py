"""Float64 geometry of a ray against every leaf of a pool, with a margin for what the f32 walk
may get wrong -- the reference of tests/test_geometry_model.py and tests/test_gpu_geometry.py.
Plain numpy; it calls neither the oracle nor the library (only the builder, for the pools).

A ray is taken as traced: query.sanitize_rays output, o' = o / 32 + 1.5 and d in float64.  Leaf
(L, ix, iy, iz) is the box [1 + i 2^-L, 1 + (i + 1) 2^-L]^3.  Per ray i the margin is

    m_i = K * 2^-23 * max(1, |o'|_inf)        (SVO units)

and, per ray,  may  = leaves whose box grown by m_i the ray touches (t >= 0),
               must = leaves whose box shrunk by m_i the ray crosses over a positive length
                      (none when size <= 2 m_i); in the HLSL stack mode only those whose shrunk
                      crossing is longer than 2^-17 * t_exit.
A ray is decided when its earliest may leaf (by grown entry) is a must leaf and no other may leaf
enters (grown) before that leaf's shrunk entry: then the answer is that leaf whatever the rounding.

Derivation of K (u = 2^-24, the unit roundoff; nothing here is fitted to a tracer's output)
--------------------------------------------------------------------------------------------
The walk (NVIDIASVO.compute:15-54, oracle/svo_oracle.c) decides everything by comparing values
t^(X) = fl(fl(X c^) - b^) of the planes X in [1, 2] of the mirrored cube, where per axis
    o^ = o' (1 + e0)            the world -> SVO transform: o / 32 is exact, the + 1.5 rounds
    c^ = c (1 + e1)             coef = 1 / -|d|
    b^ = c^ o^ (1 + e2)         bias, d < 0
    b^ = (3 c^ (1 + e5) - c^ o^ (1 + e2)) (1 + e6)     bias, d > 0 (the mirrored axis, O = 3 - o')
    t^ = (X c^ (1 + e3) - b^) (1 + e4)                 e3 = 0 where the kernel fuses coef * x - bias
with every |e| <= u.  To first order t^ = c (X + dX - O) with a plane displacement
    d < 0:  |dX| <= u (X + 2 |o'| + 2 |X - o'|)
    d > 0:  |dX| <= u (X + 3 + 2 |o'| + |3 - o'| + 2 |X - O|)
(the relative factors (1 + e1)(1 + e4) of t act like a displacement of 2u |X - O|).  The child
selection compares t_center = fl(half * coef + t_corner): one more rounding, 3u |X - O| in all.
Over X in [1, 2] the worst case is the mirrored axis with o' = -1 (O = 4, X = 1):
    u (1 + 3 + 2 + 4 + 9) = 19 u = 9.5 * 2^-23 * max(1, |o'|),
and for |o'| -> inf the bound tends to 3 * 2^-23 |o'|; in between it is below 9.5 (d < 0 peaks
at 6.5, o' = -1).  K = 10 covers it with 0.5 * 2^-23 for the second-order terms (~ 50 u^2).
Stack, positions and sizes are exact in EXACT mode (dyadic); t_min and t_max are copies of
such t^ values.  The HLSL stack stores asint(t_max) ~ 2^30 through a float: 24 significant bits,
so a popped t_max is off by up to 2^-17 t_max (t_max >= 2) or 2^-18 t_max (below): rounded down
it hides a child whose crossing is shorter than that, rounded up it changes nothing (the
child's own tc_max still bounds the span).  Rounding an already rounded value is exact, so the
error does not compound over levels.

What the margin cannot see: a must crossing is longer than 2 m_i, so its f32 span is strictly positive
and the span test t_min <= tv_max could be < without any must leaf being lost -- the two differ only on
crossings thinner than the rounding error, where geometry prefers neither.  That convention (closed
spans, the reference's) is pinned by the byte-for-byte parity tests against the oracle, not here.  For
the same reason pools whose voxels are at most 2 m_i wide (depth 19: 16 * 2^-23, depth 21: 4 * 2^-23) have
no must leaf and no decided ray: they get safety, scale, key, entry distance, flags and the misses.
The decided share is taken over the rays with a non-empty may set (a model miss has nothing to decide).

The entry-distance assertion compares t / 2048 with the leaf's slab entry max_k t_near_k
(clamped at 0) within m_i / min |d_k|: every plane moves by at most m_i, so every t_near_k by at
most m_i / |d_k|.  (The grown box's entry lies m_i / |d_k| before it by construction; a band of the
same width centred there would cut off the true value.)
"""
import functools

import numpy as np

from raytracingtest_amd.builder import build_from_leaves, build_menger
from raytracingtest_amd.camera import Camera, look_rotation, main_light
from raytracingtest_amd.query import camera_rays, make_rays, sanitize_rays
from raytracingtest_amd.svo_data import SVOData

ULP = 2.0 ** -23
K = 10.0
HLSL_REL = 2.0 ** -17
EXACT, HLSL = 1, 0                      # svo_stack_mode values
FLAG_HIT, FLAG_CAP, FLAG_OVERFLOW = 1, 2, 4
WALK_DEPTHS = (7, 12, 16, 19, 21)
# walk14 .. walk18: the secondary-ray tests' depths (tests/secondary_geometry_model.py); appended, because
# family_rays seeds by a pool's index here
POOLS = ("walk7", "menger7", "walk12", "mixed", "walk16", "walk19", "walk21", "walk14", "walk15", "walk17", "walk18")
FAMILIES = ("far", "near", "mid", "surface", "slanted", "camera")
DECIDED_FLOOR = {"walk7": 0.99, "menger7": 0.99, "walk12": 0.95, "mixed": 0.95, "walk16": 0.40}
CAM_W, CAM_H = 128, 96


def cam_size(name):
    """The camera family's frame: 128 x 96, on the 462k-leaf sponge 32 x 24 (rays x leaves in float64)."""
    return (32, 24) if name == "menger7" else (CAM_W, CAM_H)
SHADOW_OFFSET = 0.001 / 32.0            # the shadow ray's origin offset in SVO units
N_RAYS = 1000


# --------------------------------------------------------------------------------------- pools
def walk_leaves(depth, seed=1234, clusters=40, steps=40):
    """40 clusters of 40-step random walks on the 2^depth grid: starts in [8, N - 8)^3, steps in
    {-1, 0, 1}^3, clipped to the grid; the unique cells (about 1,400)."""
    rng = np.random.default_rng(seed)
    n = 1 << depth
    cells = []
    for _ in range(clusters):
        p = rng.integers(8, n - 8, 3)
        for _ in range(steps):
            cells.append(p.copy())
            p = np.clip(p + rng.integers(-1, 2, 3), 0, n - 1)
    return np.unique(np.array(cells, np.int64), axis=0)


def _walk_pool(depth):
    xyz = walk_leaves(depth)
    nrm = np.random.default_rng(depth).normal(size=(len(xyz), 3)).astype(np.float32)
    return build_from_leaves(depth, xyz, nrm)


def _mixed_pool():
    """The depth-12 walk pool with the non-leaf byte cleared (tests/lod_util.pruned's way) on a
    seeded third of the level-10 and level-11 descriptors: leaves at depths 10, 11 and 12."""
    svo = _walk_pool(12).as_v2()
    level = svo.levels()
    rng = np.random.default_rng(77)
    nodes = svo.nodes.copy()
    for l in (10, 11):
        at = np.flatnonzero(level == l)
        nodes[rng.choice(at, len(at) // 3, replace=False)] &= ~np.uint64(0xFF)
    return SVOData(nodes=nodes, attachments=svo.attachments)


@functools.lru_cache(maxsize=None)
def pool(name):
    """(SVOData, leaves): leaves = SVOData.leaf_voxels() rows (node, slot, L, ix, iy, iz), read-only."""
    if name == "menger7":
        svo = build_menger(7)
    elif name == "mixed":
        svo = _mixed_pool()
    else:
        svo = _walk_pool(int(name[4:]))
    leaves = svo.leaf_voxels()
    leaves.setflags(write=False)
    return svo, leaves


def boxes(leaves):
    size = 2.0 ** -leaves[:, 2].astype(np.float64)
    lo = 1.0 + leaves[:, 3:6].astype(np.float64) * size[:, None]
    return lo, lo + size[:, None], size


def voxel_keys(leaves):
    """ix | iy << 21 | iz << 42: the key's coordinates are the corner's 23-bit mantissa >> scale,
    which are the leaf's integer coordinates at its depth L = 23 - scale."""
    c = leaves[:, 3:6].astype(np.uint64)
    return c[:, 0] | (c[:, 1] << np.uint64(21)) | (c[:, 2] << np.uint64(42))


# ---------------------------------------------------------------------------------------- rays
def svo_rays(rays):
    """(o', d, m) in float64 of rays as traced (sanitize_rays output)."""
    o = rays["origin"].astype(np.float64) / 32.0 + 1.5
    d = rays["dir"].astype(np.float64)
    m = K * ULP * np.maximum(1.0, np.abs(o).max(axis=1))
    return o, d, m


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _world(o_svo, d):
    return make_rays(((o_svo - 1.5) * 32.0).astype(np.float32), d.astype(np.float32))


def _targets(rng, leaves, n, inset=0.1):
    lo, hi, size = boxes(leaves)
    k = rng.integers(0, len(leaves), n)
    f = rng.uniform(inset, 1.0 - inset, (n, 3))
    return k, lo[k] + f * size[k, None], size[k]


def _candidates(name, family, rng, count, aimed):
    """count rays of a family: aimed at their target point, or strays (the same rule for the origins,
    an unrelated direction)."""
    _, leaves = pool(name)
    k, p, size = _targets(rng, leaves, count)
    u = _unit(rng, count)
    if family == "slanted":
        a = rng.integers(0, 3, count)
        u[np.arange(count), a] = 0.0
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        u[np.arange(count), a] = 1e-3 * rng.choice([-1.0, 1.0], count)
    if family == "far":
        s = rng.uniform(2.0, 4.0, count)
    elif family == "mid":
        s = rng.uniform(0.05, 0.4, count)
    else:                                   # near, slanted: 3 to 40 voxel sizes
        s = rng.uniform(3.0, 40.0, count) * size
    o = p - s[:, None] * u
    d = u if aimed else _unit(rng, count)
    if not aimed and family == "slanted":
        d = u * rng.choice([-1.0, 1.0], (count, 3))
    return _world(o, d)


def _surface(name, seed, n):
    """Origins on a leaf face pushed outward by the shadow offset or half a voxel, directions in the
    outward hemisphere: the starts of secondary rays."""
    _, leaves = pool(name)
    rng = np.random.default_rng(seed)
    lo, hi, size = boxes(leaves)
    k = rng.integers(0, len(leaves), n)
    p = lo[k] + rng.uniform(0.0, 1.0, (n, 3)) * size[k, None]
    axis, sign = rng.integers(0, 3, n), rng.choice([-1.0, 1.0], n)
    delta = np.where(np.arange(n) % 2 == 0, SHADOW_OFFSET, 0.5 * size[k])
    r = np.arange(n)
    p[r, axis] = np.where(sign > 0, hi[k, axis], lo[k, axis]) + sign * delta
    d = _unit(rng, n)
    d[r, axis] = np.abs(d[r, axis]) * sign
    return _world(p, d), k


def camera(name):
    """A narrow view (11 degrees) of the pool's first cluster from 200 voxel sizes away; the GPU leg renders it."""
    _, leaves = pool(name)
    lo, hi, size = boxes(leaves)
    centre = 0.5 * (lo[0] + hi[0])
    vox = size.min()
    near = np.abs(0.5 * (lo + hi) - centre).max(axis=1) < 24 * vox
    target = (0.5 * (lo + hi))[near].mean(axis=0)
    off = np.array([0.48, 0.55, -0.68])
    if name == "menger7":               # dense: a corner that faces the light, from outside in the plane of
        sgn = np.where(-main_light()[:3] > 0, 1.0, -1.0)         # one of its faces: half the frame is sky
        target, off = np.where(sgn > 0, hi.max(axis=0), lo.min(axis=0)), sgn * np.array([0.6, 0.8, 0.0])
    off /= np.linalg.norm(off)
    eye = target + 200.0 * vox * off
    fov = np.rad2deg(2.0 * np.arctan(10.0 / 200.0))
    return Camera(position=tuple((eye - 1.5) * 32.0), rotation=look_rotation(target - eye), fov=float(fov))


@functools.lru_cache(maxsize=None)
def family_rays(name, family):
    """(rays, start_leaf): the seeded batch of a family on a pool, read-only.  Aimed families hold
    N_RAYS aimed rays plus up to N_RAYS / 4 strays chosen by the model alone (125 model misses where
    the search finds them, so that truth is never 'all hit', and up to 125 others); surface rays are
    chosen the same way.  start_leaf: the leaf row a surface ray starts on, else -1."""
    seed = 1000 * POOLS.index(name) + FAMILIES.index(family)
    if family == "camera":
        w, h = cam_size(name)
        rays = camera_rays(*camera(name).uniforms(w, h), w, h)
        start = np.full(len(rays), -1)
    elif family == "surface":
        rays, start = _surface(name, seed, 5 * N_RAYS // 2)
        empty = model(name, sanitize_rays(rays[N_RAYS:])[0])[EXACT]["n_may"] == 0
        keep = np.concatenate([np.arange(N_RAYS), N_RAYS + np.flatnonzero(empty)[:N_RAYS // 8],
                               N_RAYS + np.flatnonzero(~empty)[:N_RAYS // 8]])
        rays, start = rays[keep], start[keep]
    else:
        rng = np.random.default_rng(seed)
        parts, misses, others = [_candidates(name, family, rng, N_RAYS, True)], 0, 0
        for _ in range(16):                      # strays in blocks, until 125 of them are model misses
            stray = _candidates(name, family, rng, 500, False)
            empty = model(name, sanitize_rays(stray)[0])[EXACT]["n_may"] == 0
            keep = np.zeros(len(stray), bool)
            keep[np.flatnonzero(empty)[:N_RAYS // 8 - misses]] = True
            keep[np.flatnonzero(~empty)[:N_RAYS // 8 - others]] = True
            misses, others = misses + int((keep & empty).sum()), others + int((keep & ~empty).sum())
            parts.append(stray[keep])
            if misses >= N_RAYS // 8:
                break
        rays = np.concatenate(parts)
        start = np.full(len(rays), -1)
    rays.setflags(write=False)
    return rays, start


# --------------------------------------------------------------------------------------- model
def _slabs(lo, hi, o, d, m):
    """Per (ray, leaf, axis): slab entry / exit of the true box and the per-axis margin in t.
    o, d: [R, 1, 3]; lo, hi: [1 or R, L, 3]; m: [R, 1, 1]."""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        t0, t1 = (lo - o) * inv, (hi - o) * inv
        mt = m * np.abs(inv)
    return np.minimum(t0, t1), np.maximum(t0, t1), mt


def _gap(tn, tf, d):
    """The least growth of the box at which the ray (t >= 0) touches it: its distance from the ray in the
    per-axis (L-infinity) sense the margin is stated in.  tn, tf: [R, L, 3] slab entries / exits."""
    with np.errstate(divide="ignore", invalid="ignore"):
        w = 1.0 / np.abs(d)                                   # t per unit of growth, per axis
        g = np.zeros(tn.shape[:2])
        for k in range(3):
            g = np.maximum(g, np.where(np.isfinite(tf[..., k]), -tf[..., k] / w[..., k], 0.0))
            for j in range(3):
                if j != k:
                    num = tn[..., j] - tf[..., k]
                    g = np.maximum(g, np.where(np.isfinite(num), num / (w[..., j] + w[..., k]), 0.0))
    return g


def _crossings(lo, hi, size, o, d, m, gap=False, t_lim=None):
    """Grown and shrunk crossings of every (ray, leaf): dict of [R, L] arrays.  may, entry_g: the grown
    box (entry clamped at 0, inf off the ray); entry_s, exit_s: the shrunk box; must[mode]; entry_true:
    the box's own slab entry (clamped at 0); axis_d: |d| of the axis it enters through.  t_lim [R]: the
    rays end there -- a leaf is a may leaf only if its grown crossing begins inside [0, t_lim], a must leaf
    only if its shrunk crossing has a positive length inside it (the stack-rounding condition of the HLSL
    mode stays one on the whole crossing: it is about what the walk descends into, not about the filter)."""
    o, d, m3 = o[:, None, :], d[:, None, :], m[:, None, None]
    tn, tf, mt = _slabs(lo, hi, o, d, m3)
    par = np.broadcast_to(d == 0.0, tn.shape)
    if par.any():       # a zero component: inside the (grown / shrunk) slab -> unbounded, else never
        in_g = (o >= lo - m3) & (o <= hi + m3)
        in_s = (o > lo + m3) & (o < hi - m3)
        mt = np.where(par, 0.0, mt)
        tn_g, tf_g = np.where(par, np.where(in_g, -np.inf, np.inf), tn), np.where(par, np.where(in_g, np.inf, -np.inf), tf)
        tn_s, tf_s = np.where(par, np.where(in_s, -np.inf, np.inf), tn), np.where(par, np.where(in_s, np.inf, -np.inf), tf)
    else:
        tn_g = tn_s = tn
        tf_g = tf_s = tf
    te_g, tx_g = (tn_g - mt).max(axis=2), (tf_g + mt).min(axis=2)
    te_s, tx_s = (tn_s + mt).max(axis=2), (tf_s - mt).min(axis=2)
    may = (te_g <= tx_g) & (tx_g >= 0.0)
    entry_g = np.where(may, np.maximum(te_g, 0.0), np.inf)
    entry_s = np.maximum(te_s, 0.0)
    slack = HLSL_REL * np.maximum(tx_s, 0.0)
    with np.errstate(invalid="ignore"):
        cross = np.where((size > 2.0 * m[:, None]) & np.isfinite(tx_s - entry_s), tx_s - entry_s, -np.inf)
    k = tn_g.argmax(axis=2)
    extra = {"gap": _gap(tn, tf, d)} if gap else {}
    must = {EXACT: cross > 0.0, HLSL: cross > slack}
    if t_lim is not None:
        tl = np.asarray(t_lim, np.float64)[:, None]
        may = may & (np.maximum(te_g, 0.0) <= tl)
        entry_g = np.where(may, entry_g, np.inf)
        with np.errstate(invalid="ignore"):
            inside = np.minimum(tx_s, tl) - entry_s > 0.0
        must = {mode: v & inside for mode, v in must.items()}
    return {**extra, "may": may, "must": must, "entry_g": entry_g, "entry_s": entry_s, "exit_s": tx_s,
            "entry_true": np.maximum(tn_g.max(axis=2), 0.0), "slack": slack,
            "axis_d": np.take_along_axis(np.broadcast_to(np.abs(d), tn_g.shape), k[..., None], axis=2)[..., 0]}


def _summarise(c, mode, index=None):
    """Per-ray summary of a _crossings block in one stack mode; index maps its leaf columns to leaf rows."""
    must = c["must"][mode]
    r = np.arange(len(c["may"]))
    n_may, n_must = c["may"].sum(axis=1), must.sum(axis=1)
    entry_s = np.where(must, c["entry_s"], np.inf)
    first = c["entry_g"].argmin(axis=1)
    others = c["entry_g"].copy()
    others[r, first] = np.inf
    decided = (n_may > 0) & must[r, first] & (others.min(axis=1) >= entry_s[r, first])
    fm = entry_s.argmin(axis=1)
    slack = c["slack"][r, fm] if mode == HLSL else np.zeros(len(r))
    col = (lambda a: a) if index is None else (lambda a: index[a])
    return {"n_may": n_may, "n_must": n_must, "first": np.where(n_may > 0, col(first), -1), "decided": decided,
            "must_entry": entry_s[r, fm], "must_slack": np.where(n_must > 0, slack, 0.0),
            "first_must": np.where(n_must > 0, col(fm), -1),
            # for a union of several pools' sets (tests/scene_geometry_model.py): the earliest may leaf's grown
            # entry, whether it is a must leaf and where its shrunk crossing begins, and the next grown entry
            "first_entry": c["entry_g"][r, first], "first_is_must": must[r, first] & (n_may > 0),
            "first_entry_s": entry_s[r, first], "other_entry": others.min(axis=1)}


def _no_leaf(n):
    z = np.zeros(n)
    return {"n_may": z.astype(np.int64), "n_must": z.astype(np.int64), "first": z.astype(np.int64) - 1,
            "decided": z.astype(bool), "must_entry": z + np.inf, "must_slack": z.copy(), "first_must": z.astype(np.int64) - 1,
            "first_entry": z + np.inf, "first_is_must": z.astype(bool), "first_entry_s": z + np.inf, "other_entry": z + np.inf}


def cells_of(leaves):
    """Leaves grouped by the cell of their ancestor three levels up (at most level 4) -- a cull, a superset
    of every may set: order, offsets, cell boxes."""
    level = int(min(4, leaves[:, 2].min() - 3))
    c = leaves[:, 3:6] >> (leaves[:, 2] - level)[:, None]
    key = (c[:, 0] << 8) | (c[:, 1] << 4) | c[:, 2]
    order = np.argsort(key, kind="stable")
    uk, start = np.unique(key[order], return_index=True)
    cell = np.stack([uk >> 8, (uk >> 4) & 15, uk & 15], axis=1).astype(np.float64)
    clo = 1.0 + cell * 2.0 ** -level
    return order, np.append(start, len(order)), clo, clo + 2.0 ** -level


@functools.lru_cache(maxsize=None)
def _cells(name):
    return cells_of(pool(name)[1])


def model(name, traced):
    """model_of on a named pool for rays as traced (sanitize_rays output), the margin derived from the rays."""
    return model_of(pool(name)[1], _cells(name), *svo_rays(traced))


def model_of(leaves, cells, o, d, m, t_lim=None, skip=None):
    """Per-ray sets of rays on a leaf table: {stack mode: dict of [n] arrays} with n_may, n_must,
    first (earliest may leaf row, -1), decided (that leaf is the answer whatever the rounding),
    first_must (row, -1), must_entry (shrunk entry of the earliest must leaf, inf) and must_slack (its
    HLSL slack).  leaves: SVOData.leaf_voxels() rows; cells: cells_of(leaves); o, d [n, 3] float64: the rays in
    the table's SVO frame; m [n]: their margins; t_lim [n]: the parameter interval's end (None: unbounded);
    skip [n]: a leaf row per ray that is left out of its sets (-1: none)."""
    lo, hi, size = boxes(leaves)
    n = len(o)
    order, offs, clo, chi = cells
    inf = np.full((1, len(clo)), np.inf)
    lim = (lambda sl: None) if t_lim is None else (lambda sl: np.asarray(t_lim, np.float64)[sl])
    touched = np.concatenate([_crossings(clo[None], chi[None], inf, o[s:s + 512], d[s:s + 512], m[s:s + 512],
                                         t_lim=lim(slice(s, s + 512)))["may"]
                              for s in range(0, n, 512)]) if n and len(clo) else np.zeros((n, len(clo)), bool)
    out = {mode: _no_leaf(n) for mode in (EXACT, HLSL)}

    def crossings(idx, e):
        c = _crossings(lo[None, idx], hi[None, idx], size[None, idx], o[e], d[e], m[e], t_lim=lim(e))
        if skip is not None:
            own = idx[None, :] == np.asarray(skip)[e][:, None]
            c["may"] = c["may"] & ~own
            c["entry_g"] = np.where(own, np.inf, c["entry_g"])
            c["must"] = {mode: v & ~own for mode, v in c["must"].items()}
        return c

    def put(rows, c, index=None):
        for mode in (EXACT, HLSL):
            for k, v in _summarise(c, mode, index).items():
                out[mode][k][rows] = v

    live = np.flatnonzero(touched.any(axis=1))
    if len(leaves) <= 4096:
        for s in range(0, len(live), 256):       # neighbours in a frame touch the same few cells
            e = live[s:s + 256]
            idx = np.concatenate([order[offs[c]:offs[c + 1]] for c in np.flatnonzero(touched[e].any(axis=0))])
            put(e, crossings(idx, e), idx)
    else:
        for i in live:
            idx = np.concatenate([order[offs[c]:offs[c + 1]] for c in np.flatnonzero(touched[i])])
            j = slice(i, i + 1)
            put(j, crossings(idx, j), idx)
    return out


def pairs(name, traced, rows):
    """pairs_of on a named pool for rays as traced."""
    return pairs_of(pool(name)[1], rows, *svo_rays(traced))


def pairs_of(leaves, rows, o, d, m, t_lim=None):
    """The crossing of ray i with leaf rows[i] alone: _crossings' arrays as [n]."""
    lo, hi, size = boxes(leaves[rows])
    c = _crossings(lo[:, None], hi[:, None], size[:, None], o, d, m, gap=True, t_lim=t_lim)
    return {k: v[:, 0] for k, v in c.items() if isinstance(v, np.ndarray)}


@functools.lru_cache(maxsize=None)
def case(name, family):
    """(rays as traced, start_leaf, {mode: model summary}) of a pool and family, computed once."""
    rays, start = family_rays(name, family)
    traced, invalid = sanitize_rays(rays)
    assert not invalid.any()
    traced.setflags(write=False)
    return traced, start, model(name, traced)


def decided_share(summaries):
    """Share of the rays with a non-empty may set (there is something to decide) that are decided."""
    some = np.concatenate([s["n_may"] > 0 for s in summaries])
    return float(np.concatenate([s["decided"] for s in summaries])[some].mean())


def leaf_rows(name, hits):
    """leaf_rows_of on a named pool (uploaded at descriptor 0)."""
    return leaf_rows_of(pool(name)[1], hits)


def leaf_rows_of(leaves, hits, root=0):
    """Leaf row of every hit record (parent - root, hit_idx); AssertionError if one is no leaf of the pool."""
    code = leaves[:, 0] * 8 + leaves[:, 1]
    srt = np.argsort(code)
    want = (hits["parent"].astype(np.int64) - int(root)) * 8 + hits["hit_idx"]
    if not len(code):
        assert not len(want), "a reported voxel in an empty pool"
        return np.zeros(0, np.int64)
    pos = np.clip(np.searchsorted(code[srt], want), 0, len(code) - 1)
    bad = code[srt][pos] != want
    assert not bad.any(), f"{bad.sum()} reported voxels are no leaf of the pool, first (parent, slot) " \
                          f"{(int(hits['parent'][bad][0]) - int(root), int(hits['hit_idx'][bad][0]))}"
    return srt[pos]


# ---------------------------------------------------------------------------------- assertions
def check(name, traced, mode, summary, hits, voxel, what=""):
    """check_of on a named pool for rays as traced."""
    return check_of(pool(name)[1], *svo_rays(traced), mode, summary, hits, voxel, what=what)


def check_of(leaves, o, d, m, mode, summary, hits, voxel, what="", t_lim=None, skip=None, masks=None):
    """Section-2 assertions on any tracer's hit records and voxel keys.  Returns the figures for the
    record: rays, hits, decided share, max_gap_ulp -- the largest distance of a reported voxel from the
    float64 ray in units of 2^-23 (the margin allows K max(1, |o'|_inf) of them) -- and max_entry_dev,
    the largest deviation of t from the leaf's entry in units of 2^-23 max(1, |o'|_inf) / min |d_k| (K allowed).
    leaves, o, d, m: as model_of takes them, t_lim and skip too (the summary was made with them).  A record that
    reports its ray's skipped leaf -- the voxel a secondary ray starts on -- is a self-hit: its key and scale are
    checked, it is counted (self_hits, and empty_but_hit where the ray's may set is empty) and otherwise left
    alone.  masks: a dict that receives self_hit [n] and rows [n] (the reported leaf rows, -1 on misses)."""
    voxel = np.asarray(voxel, np.uint64)
    flags = hits["flags"]
    assert not np.any(flags & (FLAG_CAP | FLAG_OVERFLOW)), f"{what}: iteration-cap or overflow flag"
    assert not np.any(flags & ~np.uint16(FLAG_HIT)), f"{what}: unexpected flag bits {np.unique(flags)}"
    hit = (flags & FLAG_HIT) != 0
    assert np.array_equal(hit, hits["parent"] != 0xFFFFFFFF), f"{what}: hit bit and parent disagree"
    h = np.flatnonzero(hit)
    try:
        rows = leaf_rows_of(leaves, hits[h])
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None
    own = np.zeros(len(h), bool) if skip is None else rows == np.asarray(skip)[h]
    ok = ~own
    p = pairs_of(leaves, rows, o[h], d[h], m[h], t_lim=None if t_lim is None else np.asarray(t_lim, np.float64)[h])
    off = ok & ~p["may"]
    assert not off.any(), f"{what}: {np.count_nonzero(off)} reported voxels off the ray, first rays {h[off][:5]}"
    assert np.array_equal(hits["hit_scale"][h], 23 - leaves[rows, 2]), f"{what}: hit_scale != 23 - L"
    assert np.array_equal(voxel[h], voxel_keys(leaves[rows])), f"{what}: voxel key"
    assert np.all(voxel[~hit] == ~np.uint64(0)) and np.all(np.isinf(hits["t"][~hit])), f"{what}: a miss carries a key or a t"
    t = hits["t"][h].astype(np.float64) / 2048.0
    tol = m[h] / np.abs(d[h]).min(axis=1)
    dev = np.abs(t - p["entry_true"])
    bad = ok & (dev > tol)
    assert not bad.any(), f"{what}: {bad.sum()} entry distances off, worst {np.max(dev / tol):.2f} tolerances (ray {h[np.argmax(dev / tol)]})"
    late = ok & (p["entry_g"] > summary["must_entry"][h] + summary["must_slack"][h])
    assert not late.any(), f"{what}: {late.sum()} rays report a voxel behind a must leaf, first {h[late][:5]}"
    lost = (summary["n_must"] > 0) & ~hit
    assert not lost.any(), f"{what}: {lost.sum()} rays with a must leaf came back as misses, first {np.flatnonzero(lost)[:5]}"
    self_hit = np.zeros(len(hits), bool)
    self_hit[h] = own
    ghost = ~self_hit & (summary["n_may"] == 0) & (hit | (flags != 0))
    assert not ghost.any(), f"{what}: {ghost.sum()} rays with an empty may set are no plain miss, first {np.flatnonzero(ghost)[:5]}"
    wrong = ok & summary["decided"][h] & (rows != summary["first"][h])
    assert not wrong.any(), f"{what}: {wrong.sum()} decided rays report another leaf, first {h[wrong][:5]}"
    fig = {"rays": int(len(hits)), "hits": int(hit.sum()), "must": int((summary["n_must"] > 0).sum()),
           "model_misses": int((summary["n_may"] == 0).sum()),
           "decided_share": round(decided_share([summary]), 4) if (summary["n_may"] > 0).any() else 1.0,
           "max_gap_ulp": round(float(np.max(p["gap"][ok] / ULP)), 3) if ok.any() else 0.0,
           "max_entry_dev": round(float(np.max((dev / tol)[ok]) * K), 3) if ok.any() else 0.0}
    if skip is not None:
        fig.update(self_hits=int(own.sum()), empty_but_hit=int((self_hit & (summary["n_may"] == 0)).sum()))
    if masks is not None:
        full = np.full(len(hits), -1, np.int64)
        full[h] = rows
        masks.update(self_hit=self_hit, rows=full)
    return fig


# --------------------------------------------------------------------------------- shadow rays
def shadow_rays(rays, hits, light):
    """The shadow ray of every hit record as svo_rt.h defines it (SVO_OPT_SHADOW_RAYS), in f32 operation by
    operation: P = o + (t / 64) d, origin P + 0.001 n, direction -L.  rays: the primary rays of the records."""
    f = np.float32
    tw = (hits["t"] * f(1.0 / 64.0))[:, None]
    n = np.stack([hits["nx"], hits["ny"], hits["nz"]], axis=1)
    origin = (rays["origin"] + tw * rays["dir"]) + n * f(0.001)
    return make_rays(origin, np.broadcast_to(-np.asarray(light, f)[:3], origin.shape))


def check_shadow(name, rays, hits, light, mode, what=""):
    """A pixel's shadow bit (flag bit 3) must be set when its float64 shadow ray has a must leaf and clear
    when its may set is empty; the pixels in between are counted.  Returns the counts."""
    flags = hits["flags"]
    hit = (flags & FLAG_HIT) != 0
    assert not np.any(flags[~hit] & 8), f"{what}: a miss pixel carries the shadow bit"
    sr = shadow_rays(rays[hit], hits[hit], light)
    traced, invalid = sanitize_rays(sr)
    assert not invalid.any() and traced.tobytes() == sr.tobytes()      # nothing to clamp: the rays as traced
    s = model(name, traced)[mode]
    bit = (flags[hit] & 8) != 0
    must, empty = s["n_must"] > 0, s["n_may"] == 0
    assert bit[must].all(), f"{what}: {np.count_nonzero(~bit[must])} pixels whose shadow ray must hit are lit"
    assert not bit[empty].any(), f"{what}: {np.count_nonzero(bit[empty])} pixels whose shadow ray meets nothing are shadowed"
    return {"hit_pixels": int(hit.sum()), "must_shadowed": int(must.sum()), "must_lit": int(empty.sum()),
            "undecided": int((~must & ~empty).sum()), "undecided_shadowed": int(bit[~must & ~empty].sum())}
