"""The closest-voxel rule in plain numpy / Python (csrc/svo_closest.h is the native statement, INTEGRATION.md
"Closest voxels" the prose one): which result voxel of a pool is nearest to a world-space point, its squared
distance d2 and the closest point on it.

  make_queries                svo_shape records of kind sphere: the point and the search radius
  object_queries              queries in a placed svo_object's frame (overlap.object_spheres on the point)
  closest_model               the walk itself, query by query: nearest records, contacts, hit mask -- what
                              svo_closest_voxels writes, byte for byte
  result_voxels               the result voxels of a pool at a coarse_level, no pruning: rows like
                              SVOData.leaf_voxels (which it equals, up to order, at coarse_level 0)
  closest_bruteforce          the answer over all result voxels, no tree, with the rule's f32 arithmetic
  true_d2                     float64 squared distances of points to voxel rows (every input is exact in it)

Frame: the tree's own world convention, the cube [-16, 16]^3.  The root descriptor is level 0; a child at level
L with integer coordinates i has side = 2^(5 - L), lo = i side - 16, hi = lo + side, all exact in f32.

The rule.  A query is a sphere (p, q[0]); invalid under overlap.shapes_valid, and also as a box: flags 0x10,
visits 0, nothing found.  r2 = q[0] q[0], +inf with CLOSEST_UNBOUNDED.  For a voxel box [lo, hi]:
e_k = max(max(lo_k - p_k, p_k - hi_k), 0), d2 = (e0 e0 + e1 e1) + e2 e2, every operation one f32 rounding; a
candidate iff d2 <= r2.  Result voxels: a valid child whose non-leaf bit is clear, or whose level is
coarse_level (when non-zero); a non-leaf child at level 22 sets flag bit 2 and is not entered.  The answer is
the result voxel with the smallest (d2, Morton position); Morton position: a_k = i_k << (22 - level), A precedes
B iff on the axis whose a_k ^ b_k has the highest set bit (ties: z before y before x) A's coordinate is smaller.
The walk: depth-first from root; bound starts at r2 and becomes the best d2; the best is replaced iff the new
d2 is smaller, or equal and Morton-earlier; at a descriptor, repeatedly the pending (valid, not yet taken) child
with the smallest (d2_c, slot c) among those with d2_c <= bound -- the bound of that moment -- is taken.  visits
counts descriptor fetches; a fetch beyond max_visits sets flag bit 1 and ends the walk with the best so far.
Closest point: c_k = min(max(p_k, lo_k), hi_k).
"""
import numpy as np

from . import overlap as ov
from ._lib import CLOSEST_DTYPE, CLOSEST_UNBOUNDED, CONTACT_DTYPE, SHAPE_DTYPE, SHAPE_SPHERE

FLAG_FOUND, FLAG_BUDGET, FLAG_OVERFLOW, FLAG_INVALID = 1, 2, 4, 0x10
DEFAULT_VISITS, MAX_VISITS, MAX_LEVEL = ov.DEFAULT_VISITS, ov.MAX_VISITS, ov.MAX_LEVEL
D2_REL_UNITS = 11       # svo_closest.h: |d2 - D_min| and D(answer) - D_min are at most D_min * 11 * 2^-24
D2_REL_BOUND = D2_REL_UNITS * 2.0 ** -24
_F = np.float32
_INF = _F(np.inf)


def make_queries(points, radius=0.0):
    """svo_shape records of the queries: points [n, 3], search radius a scalar or [n] (ignored when the call
    is unbounded, but it must be valid)."""
    return ov.make_spheres(points, radius)


def object_queries(points, radius, obj):
    """World-space queries in the frame of a placed svo_object, for a call with root = obj["root"]: the point
    is step 2 of the object rule, the radius r 2^-k (overlap.object_spheres).  The answer's point and d2 are in
    the object's frame: world d2 = d2 4^k, world point = R (c 2^k) + position."""
    return ov.object_spheres(points, radius, obj)


def queries_valid(queries):
    """[n] bool: overlap.shapes_valid's rule, and a box is no query."""
    queries = np.ascontiguousarray(queries, SHAPE_DTYPE).reshape(-1)
    return ov.shapes_valid(queries) & (queries["kind"] == SHAPE_SPHERE)


def nothing_found(n):
    """n svo_closest records of queries that found nothing (visits and flags 0)."""
    out = np.zeros(n, CLOSEST_DTYPE)
    out["d2"] = np.inf
    out["parent"] = 0xFFFFFFFF
    return out


def morton_code(level, coords):
    """The Morton position as one integer: the bits of a_k = i_k << (22 - level) interleaved, z above y above x."""
    code = 0
    for b in range(MAX_LEVEL - 1, -1, -1):
        for k in (2, 1, 0):
            code = code << 1 | ((int(coords[k]) << (MAX_LEVEL - level)) >> b & 1)
    return code


def morton_before(level_a, a, level_b, b):
    """The rule's comparison as the header makes it: the axis of the highest differing bit decides."""
    aa = [int(a[k]) << (MAX_LEVEL - level_a) for k in range(3)]
    bb = [int(b[k]) << (MAX_LEVEL - level_b) for k in range(3)]
    axis, m = 2, aa[2] ^ bb[2]
    for k in (1, 0):
        x = aa[k] ^ bb[k]
        if m < x and m < (m ^ x):
            axis, m = k, x
    return aa[axis] < bb[axis]


def _halves_sq(p, level, coords):
    """e_k e_k of the low and the high half per axis for the children of the descriptor at (level, coords)."""
    side, half = 2.0 ** (5 - level), 2.0 ** (4 - level)
    zero = _F(0.0)
    el, eh = [], []
    for k in range(3):
        lo = _F(coords[k] * side - 16.0)
        mid, hi = _F(lo + _F(half)), _F(lo + _F(side))
        a = max(max(lo - p[k], p[k] - mid), zero)
        b = max(max(mid - p[k], p[k] - hi), zero)
        el.append(a * a)
        eh.append(b * b)
    return el, eh


def _slot_d2(el, eh, c):
    return ((eh[0] if c & 1 else el[0]) + (eh[1] if c & 2 else el[1])) + (eh[2] if c & 4 else el[2])


def closest_model(svo, queries, root=0, flags=0, max_visits=0, coarse_level=0, n_nodes=None):
    """svo_closest_voxels as the rule states it.  svo: an SVOData uploaded at offset 0 (a tree behind another
    one: pass the whole pool as one SVOData of absolute V2 nodes); n_nodes: the uploaded extent (default: the
    pool's length) -- a fetch at or past it reads the zero descriptor.  Returns (nearest [n] CLOSEST_DTYPE,
    contacts [n] CONTACT_DTYPE, hitmask [ceil(n / 64)] uint64)."""
    queries = np.ascontiguousarray(queries, SHAPE_DTYPE).reshape(-1)
    n = len(queries)
    budget = int(max_visits) or DEFAULT_VISITS
    if not (1 <= budget <= MAX_VISITS and 0 <= coarse_level <= MAX_LEVEL and not flags & ~CLOSEST_UNBOUNDED):
        raise ValueError("closest parameters out of range")
    word, first = svo.masks_and_first()
    word, first = [int(w) for w in word], [int(f) for f in first]
    n_nodes = len(word) if n_nodes is None else int(n_nodes)
    nearest = nothing_found(n)
    contacts = ov.unused_contacts(n)
    mask = np.zeros((n + 63) // 64, np.uint64)
    valid = queries_valid(queries)
    with np.errstate(all="ignore"):
        for s in range(n):
            if not valid[s]:
                nearest[s]["flags"] = FLAG_INVALID
                continue
            p = [_F(v) for v in queries[s]["p"]]
            bound = _INF if flags & CLOSEST_UNBOUNDED else queries[s]["q"][0] * queries[s]["q"][0]
            visits = fl = 0
            best = None        # (parent, slot, level, coords)
            # one frame per descriptor on the path: [node, nonleaf8, first, pending slots, level, coords, (el, eh)]
            stack, entering = [], (int(root), 0, (0, 0, 0))
            while True:
                if entering is not None:
                    node, level, coords = entering
                    entering = None
                    if visits >= budget:
                        fl |= FLAG_BUDGET
                        break
                    visits += 1
                    inside = 0 <= node < n_nodes
                    w = word[node] if inside else 0
                    stack.append([node, w & 0xFF, first[node] if inside else 0, (w >> 8) & 0xFF, level, coords,
                                  _halves_sq(p, level, coords)])
                if not stack:
                    break
                top = stack[-1]
                node, nonleaf, f0, pend, level, coords, (el, eh) = top
                pick, keep = None, 0
                for c in range(8):
                    if pend >> c & 1:
                        dc = _slot_d2(el, eh, c)
                        if dc <= bound:
                            keep |= 1 << c
                            if pick is None or dc < pick[0]:
                                pick = (dc, c)
                if pick is None:
                    stack.pop()
                    continue
                d2, c = pick
                top[3] = keep & ~(1 << c)
                child = (2 * coords[0] + (c & 1), 2 * coords[1] + (c >> 1 & 1), 2 * coords[2] + (c >> 2 & 1))
                if not (nonleaf >> c) & 1 or level + 1 == coarse_level:
                    if best is None or d2 < bound or morton_before(level + 1, child, best[2], best[3]):
                        bound = d2
                        best = (node, c, level + 1, child)
                elif level + 1 == MAX_LEVEL:
                    fl |= FLAG_OVERFLOW
                else:
                    kid = (f0 + bin(nonleaf & ((1 << c) - 1)).count("1")) & 0xFFFFFFFF
                    entering = (kid, level + 1, child)
            if best is None:
                nearest[s]["visits"], nearest[s]["flags"] = visits, fl
                continue
            node, c, level, child = best
            side = 2.0 ** (5 - level)
            lo = [_F(child[k] * side - 16.0) for k in range(3)]
            point = [min(max(p[k], lo[k]), _F(lo[k] + _F(side))) for k in range(3)]
            meta = c | (23 - level) << 8
            nearest[s] = (point, bound, node, meta, visits, fl | FLAG_FOUND)
            contacts[s] = (node, meta, child[0] | child[1] << 21 | child[2] << 42)
            mask[s // 64] |= np.uint64(1 << (s % 64))
    return nearest, contacts, mask


def result_voxels(svo, coarse_level=0, root=0):
    """The result voxels of the tree at `root` as rows (node, slot, L, ix, iy, iz), every path walked, nothing
    pruned: leaves, and with a coarse_level the non-leaf children of that level instead of what lies below."""
    word, first = svo.masks_and_first()
    rows, todo = [], [(int(root), 0, (0, 0, 0))]
    while todo:
        node, level, coords = todo.pop()
        w, f0 = int(word[node]), int(first[node])
        for c in range(8):
            if not w >> (8 + c) & 1:
                continue
            child = (2 * coords[0] + (c & 1), 2 * coords[1] + (c >> 1 & 1), 2 * coords[2] + (c >> 2 & 1))
            if not w >> c & 1 or level + 1 == coarse_level:
                rows.append((node, c, level + 1) + child)
            elif level + 1 < MAX_LEVEL:
                todo.append((f0 + bin(w & 0xFF & ((1 << c) - 1)).count("1"), level + 1, child))
    return np.array(rows, np.int64).reshape(-1, 6)


def voxel_boxes(rows):
    """(lo, hi) [m, 3] float64 of voxel rows; exact, also as float32."""
    side = 2.0 ** (5 - rows[:, 2].astype(np.float64))
    lo = rows[:, 3:6].astype(np.float64) * side[:, None] - 16.0
    return lo, lo + side[:, None]


def true_d2(rows, point):
    """[m] float64 squared distances of one point (f32 numbers, exact in float64) to the voxel rows: float64
    arithmetic on exact inputs, relative error a few 2^-53."""
    lo, hi = voxel_boxes(rows)
    p = np.asarray(point, np.float64)
    e = np.maximum(np.maximum(lo - p, p - hi), 0.0)
    return (e * e).sum(axis=1)


def closest_bruteforce(rows, queries, flags=0):
    """The answer over all result voxels `rows` (SVOData.leaf_voxels(), or result_voxels at a coarse_level), no
    tree: d2 with the rule's f32 operations, the minimum of (d2, Morton position).  Returns (nearest, contacts)
    like closest_model, with visits 0 and the budget and overflow flags unset."""
    queries = np.ascontiguousarray(queries, SHAPE_DTYPE).reshape(-1)
    lo, hi = voxel_boxes(rows)
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    assert (lo32 == lo).all() and (hi32 == hi).all()
    nearest, contacts = nothing_found(len(queries)), ov.unused_contacts(len(queries))
    valid = queries_valid(queries)
    with np.errstate(all="ignore"):
        for s in range(len(queries)):
            if not valid[s]:
                nearest[s]["flags"] = FLAG_INVALID
                continue
            p, r = queries[s]["p"], queries[s]["q"][0]
            r2 = _INF if flags & CLOSEST_UNBOUNDED else r * r
            e = np.maximum(np.maximum(lo32 - p, p - hi32), _F(0.0))
            sq = e * e
            d2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
            cand = np.flatnonzero(d2 <= r2)
            if not len(cand):
                continue
            tied = cand[d2[cand] == d2[cand].min()]
            j = min(tied, key=lambda t: morton_code(int(rows[t, 2]), rows[t, 3:6]))
            node, c, level = (int(v) for v in rows[j, :3])
            meta = c | (23 - level) << 8
            nearest[s] = (np.minimum(np.maximum(p, lo32[j]), hi32[j]), d2[j], node, meta, 0, FLAG_FOUND)
            contacts[s] = (node, meta, int(rows[j, 3]) | int(rows[j, 4]) << 21 | int(rows[j, 5]) << 42)
    return nearest, contacts


__all__ = ["CLOSEST_DTYPE", "CLOSEST_UNBOUNDED", "CONTACT_DTYPE", "SHAPE_DTYPE", "make_queries", "object_queries",
           "queries_valid", "nothing_found", "closest_model", "result_voxels", "closest_bruteforce", "true_d2",
           "voxel_boxes", "morton_code", "morton_before"]
