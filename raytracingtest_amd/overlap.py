"""The overlap rule in plain numpy / Python (csrc/svo_overlap.h is the native statement, INTEGRATION.md
"Volume queries" the prose one): which voxels of a pool does a world-space box or sphere touch.

  make_boxes / make_spheres   svo_shape records
  object_spheres              spheres in a placed svo_object's frame (step 2 of the object rule on the centre)
  overlap_model               the walk itself, shape by shape: summaries, contacts, hit mask -- what
                              svo_overlap_volumes writes, byte for byte
  overlap_bruteforce          the count over all leaves, no tree: float64 for boxes (the numbers are exact in
                              it), the rule's f32 arithmetic for spheres

Frame: the tree's own world convention, the cube [-16, 16]^3.  The root descriptor is level 0; a child at level
L with integer coordinates i has side = 2^(5 - L), lo = i side - 16, hi = lo + side, all exact in f32.
"""
import numpy as np

from ._lib import CONTACT_DTYPE, OBJECT_DTYPE, OVERLAP_ANY, OVERLAP_DTYPE, SHAPE_BOX, SHAPE_DTYPE, SHAPE_SPHERE

FLAG_TOUCH, FLAG_BUDGET, FLAG_OVERFLOW, FLAG_INVALID = 1, 2, 4, 0x10
MAX_CONTACTS = 32
DEFAULT_VISITS, MAX_VISITS = 65536, 1 << 24
MAX_LEVEL = 22          # a non-leaf child at this level is not entered: the guarded ray walk's depth limit
_F = np.float32


def make_boxes(lo, hi):
    """svo_shape records of the closed boxes [lo, hi] ([n, 3] each, world space)."""
    lo = np.asarray(lo, np.float32).reshape(-1, 3)
    out = np.zeros(len(lo), SHAPE_DTYPE)
    out["p"] = lo
    out["q"] = np.asarray(hi, np.float32).reshape(-1, 3)
    out["kind"] = SHAPE_BOX
    return out


def make_spheres(centre, radius):
    """svo_shape records of spheres: centre [n, 3], radius a scalar or [n] (world space)."""
    centre = np.asarray(centre, np.float32).reshape(-1, 3)
    out = np.zeros(len(centre), SHAPE_DTYPE)
    out["p"] = centre
    out["q"][:, 0] = np.broadcast_to(np.asarray(radius, np.float32), (len(centre),))
    out["kind"] = SHAPE_SPHERE
    return out


def object_spheres(centre, radius, obj):
    """World-space spheres in the frame of a placed svo_object (an OBJECT_DTYPE record), for a query with
    root = obj["root"]: the centre is step 2 of the object rule applied to a point, q = c - p,
    c'_j = ((R_0j q_0 + R_1j q_1) + R_2j q_2) 2^-k, every operation one f32 rounding; the radius is r 2^-k
    (exact).  The sphere stays a sphere under the object's rotation; a box does not (out of scope)."""
    obj = np.asarray(obj, OBJECT_DTYPE).reshape(-1)[0]
    s = _F(2.0) ** _F(-int(obj["scale_log2"]))
    R = obj["rotation"].astype(_F)
    p = obj["position"].astype(_F)
    c = np.asarray(centre, np.float32).reshape(-1, 3)
    out = np.zeros((len(c), 3), np.float32)
    with np.errstate(all="ignore"):
        q = (c - p[None, :]).astype(_F)
        for j in range(3):
            a = R[j] * q[:, 0]
            a = a + R[3 + j] * q[:, 1]
            a = a + R[6 + j] * q[:, 2]
            out[:, j] = (a * s).astype(_F)
        r = (np.broadcast_to(np.asarray(radius, np.float32), (len(c),)) * s).astype(_F)
    return make_spheres(out, r)


def shapes_valid(shapes):
    """[n] bool: a shape is invalid with a non-finite number among p and q, p_k > q_k in a box, a negative
    radius or an unknown kind."""
    shapes = np.ascontiguousarray(shapes, SHAPE_DTYPE).reshape(-1)
    ok = np.isfinite(shapes["p"]).all(axis=1) & np.isfinite(shapes["q"]).all(axis=1)
    box, sphere = shapes["kind"] == SHAPE_BOX, shapes["kind"] == SHAPE_SPHERE
    with np.errstate(invalid="ignore"):
        ok &= np.where(box, ~(shapes["p"] > shapes["q"]).any(axis=1), sphere & ~(shapes["q"][:, 0] < 0))
    return ok


def unused_contacts(n):
    out = np.zeros(n, CONTACT_DTYPE)
    out["parent"] = 0xFFFFFFFF
    out["key"] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return out


def _sphere_touch(lo, hi, p, r2):
    """The sphere test on one node box, every operation one f32 rounding (numpy float32 scalars)."""
    zero = _F(0.0)
    sq = []
    for k in range(3):
        e = max(max(lo[k] - p[k], p[k] - hi[k]), zero)
        sq.append(e * e)
    return bool((sq[0] + sq[1]) + sq[2] <= r2)


def _child_touches(kind, p, q, r2, level, coords):
    """The touch test on the child at `level` with integer coordinates `coords`.  Box: p, q Python floats
    (the numbers are exact, so they compare as f32 does); sphere: p numpy float32 scalars."""
    side = 2.0 ** (5 - level)
    if kind == SHAPE_BOX:
        for k in range(3):
            lo = coords[k] * side - 16.0
            if not (lo <= q[k] and lo + side >= p[k]):
                return False
        return True
    lo = [_F(coords[k] * side - 16.0) for k in range(3)]
    hi = [_F(coords[k] * side - 16.0 + side) for k in range(3)]
    return _sphere_touch(lo, hi, p, r2)


def overlap_model(svo, shapes, root=0, max_contacts=0, flags=0, max_visits=0, coarse_level=0, n_nodes=None):
    """svo_overlap_volumes as the rule states it.  svo: an SVOData uploaded at offset 0 (a tree behind another
    one: pass the whole pool as one SVOData of absolute V2 nodes); n_nodes: the uploaded extent (default: the
    pool's length) -- a fetch at or past it reads the zero descriptor.  Returns (summary [n] OVERLAP_DTYPE,
    contacts [n, max_contacts] CONTACT_DTYPE, hitmask [ceil(n / 64)] uint64)."""
    shapes = np.ascontiguousarray(shapes, SHAPE_DTYPE).reshape(-1)
    n = len(shapes)
    K = int(max_contacts)
    budget = int(max_visits) or DEFAULT_VISITS
    if not (0 <= K <= MAX_CONTACTS and 1 <= budget <= MAX_VISITS and 0 <= coarse_level <= MAX_LEVEL and not flags & ~OVERLAP_ANY):
        raise ValueError("overlap parameters out of range")
    word, first = svo.masks_and_first()
    word, first = [int(w) for w in word], [int(f) for f in first]
    n_nodes = len(word) if n_nodes is None else int(n_nodes)
    summary = np.zeros(n, OVERLAP_DTYPE)
    contacts = unused_contacts(n * K).reshape(n, K)
    mask = np.zeros((n + 63) // 64, np.uint64)
    valid = shapes_valid(shapes)
    with np.errstate(all="ignore"):
        for s in range(n):
            if not valid[s]:
                summary[s]["flags"] = FLAG_INVALID
                continue
            shape = shapes[s]
            kind = int(shape["kind"])
            r2 = shape["q"][0] * shape["q"][0]
            p = [float(v) for v in shape["p"]] if kind == SHAPE_BOX else [_F(v) for v in shape["p"]]
            q = [float(v) for v in shape["q"]]
            count = visits = fl = 0
            # one frame per descriptor being scanned: [node, word, first, next slot, level, coordinates]
            stack, entering, done = [], (int(root), 0, (0, 0, 0)), False
            while not done:
                if entering is not None:
                    node, level, coords = entering
                    entering = None
                    if visits >= budget:
                        fl |= FLAG_BUDGET
                        break
                    visits += 1
                    inside = 0 <= node < n_nodes
                    stack.append([node, word[node] if inside else 0, first[node] if inside else 0, 0, level, coords])
                if not stack:
                    break
                top = stack[-1]
                node, w, f0, c, level, coords = top
                if c == 8:
                    stack.pop()
                    continue
                top[3] = c + 1
                if not (w >> (8 + c)) & 1:
                    continue
                child = (2 * coords[0] + (c & 1), 2 * coords[1] + (c >> 1 & 1), 2 * coords[2] + (c >> 2 & 1))
                if not _child_touches(kind, p, q, r2, level + 1, child):
                    continue
                nonleaf = w & 0xFF
                if not (nonleaf >> c) & 1 or level + 1 == coarse_level:
                    count += 1
                    if count <= K:
                        contacts[s, count - 1] = (node, c | (23 - (level + 1)) << 8,
                                                  child[0] | child[1] << 21 | child[2] << 42)
                    done = bool(flags & OVERLAP_ANY)
                elif level + 1 == MAX_LEVEL:
                    fl |= FLAG_OVERFLOW
                else:
                    kid = (f0 + bin(nonleaf & ((1 << c) - 1)).count("1")) & 0xFFFFFFFF
                    entering = (kid, level + 1, child)
            if count:
                fl |= FLAG_TOUCH
                mask[s // 64] |= np.uint64(1 << (s % 64))
            summary[s] = (count, visits, fl, 0)
    return summary, contacts, mask


def overlap_bruteforce(leaves, shapes):
    """[n] counts of the leaves each shape touches, no tree: leaves = SVOData.leaf_voxels() rows (node, slot, L,
    ix, iy, iz).  Boxes in float64 (every number is exact in it), spheres with the rule's f32 operations.
    Invalid shapes count 0."""
    shapes = np.ascontiguousarray(shapes, SHAPE_DTYPE).reshape(-1)
    side = 2.0 ** (5 - leaves[:, 2].astype(np.float64))
    lo = leaves[:, 3:6].astype(np.float64) * side[:, None] - 16.0
    hi = lo + side[:, None]
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    assert (lo32 == lo).all() and (hi32 == hi).all()
    valid = shapes_valid(shapes)
    out = np.zeros(len(shapes), np.int64)
    with np.errstate(all="ignore"):
        for s in np.flatnonzero(valid):
            sh = shapes[s]
            if sh["kind"] == SHAPE_BOX:
                p, q = sh["p"].astype(np.float64), sh["q"].astype(np.float64)
                out[s] = np.count_nonzero(((lo <= q) & (hi >= p)).all(axis=1))
            else:
                p, r = sh["p"], sh["q"][0]
                e = np.maximum(np.maximum(lo32 - p, p - hi32), _F(0.0))
                sq = e * e
                d2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
                out[s] = np.count_nonzero(d2 <= r * r)
    return out
