"""Plain numpy models of the beam starts' pieces, written from the rules stated in
csrc/svo_beam.h, csrc/svo_traverse.h (BeamParams, tile_start) and the comment above
svo_kernel.hip's beam_splat_kernel -- not ports of the code:

  splat_list_model     the splat list of a pool (svo_beam.h build_beam_boxes), exact
  beam_camera_model    the splat's view of a camera (svo_beam.h beam_camera), float64
  splat_model          per tile an envelope [lo_rule, hi_rule] of the bound the splat kernel must leave,
                       and hi_geo, the bound pure geometry demands

tests/test_beam_model.py pins these by hand; tests/test_beam_host.py and tests/test_gpu_beam_splat.py
compare the host code and the kernel with them."""
import numpy as np

GUARD = 0xA5C3F00D
GUARD_WORDS = 64
MAGIC = 0x31505342          # "BSP1": tests/beam_splat_driver.cpp
HOST_MAGIC = 0x31484D42     # "BMH1": tests/beam_host_driver.cpp
STEP_WORDS = 25             # gen, org[3], minv[9], plane[12]
MG = 0.05                   # the kernel's pixel margin around a projected box
DELTA = 0.02                # pixels the kernel's f32 projection may differ from float64 (proj_err stays below)
REL = 2.0 ** -21            # d_rule against the kernel's f32 distance: two squares, two adds, a 1-ulp sqrt <= 4 * 2^-24, doubled
INF = np.inf


# ------------------------------------------------------------------ splat list
def _spread16(v):
    out = 0
    for b in range(16):
        out |= ((v >> b) & 1) << (3 * b)
    return out


def morton16(x, y, z, d):
    """The sort key: the box's lower corner at 16 bits per axis, bits interleaved x lowest."""
    sh = 16 - d
    return _spread16(x << sh) | _spread16(y << sh) << 1 | _spread16(z << sh) << 2


def splat_list_model(lo, first, depth, back, budget=1 << 23):
    """The splat list as rows (x, y, z, depth) in Morton order, or None.  ds = min(depth - back, 16); the
    valid children at depth ds and the valid leaf children above it; child c sits in the upper half on axis
    k iff bit k of c is set, its node is first + (non-leaf slots below c); a node index >= n is an empty
    descriptor.  The budget is a rule on the level order: a node whose turn comes when the boxes listed plus
    the nodes already queued for the next level have reached the budget lists its valid children as boxes."""
    lo = [int(v) for v in lo]
    first = [int(v) for v in first]
    n = len(lo)
    ds = min(depth - back, 16)
    if ds < 1 or n == 0:
        return None
    boxes = []

    def level(nodes, d):   # nodes: (index, x, y, z) of the non-leaf nodes whose children are at depth d + 1
        if not nodes or d == ds:
            return
        queued = []
        for node, x, y, z in nodes:
            inner, valid = lo[node] & 0xFF, (lo[node] >> 8) & 0xFF
            open_ = len(queued) + len(boxes) < budget
            for c in range(8):
                if not (valid >> c) & 1:
                    continue
                pos = (2 * x + (c & 1), 2 * y + ((c >> 1) & 1), 2 * z + ((c >> 2) & 1))
                if (inner >> c) & 1 and d + 1 < ds and open_:
                    child = first[node] + bin(inner & ((1 << c) - 1)).count("1")
                    if child < n:
                        queued.append((child,) + pos)
                else:
                    boxes.append(pos + (d + 1,))
        level(queued, d + 1)

    level([(0, 0, 0, 0)], 0)
    boxes.sort(key=lambda b: morton16(*b))
    return np.array(boxes, np.int64).reshape(-1, 4)


def box_words(rows):
    """(x, y, z, depth) rows -> the (x | y << 16, z | depth << 16) words."""
    r = np.asarray(rows, np.int64).reshape(-1, 4)
    return np.stack([r[:, 0] | (r[:, 1] << 16), r[:, 2] | (r[:, 3] << 16)], axis=1).astype(np.uint32)


def box_rows(words):
    w = np.asarray(words, np.uint32).reshape(-1, 2).astype(np.int64)
    return np.stack([w[:, 0] & 0xFFFF, w[:, 0] >> 16, w[:, 1] & 0xFFFF, w[:, 1] >> 16], axis=1)


def positional_leaves(lo, first):
    """Every leaf voxel (x, y, z, level) by position, shared subtrees once per position (what
    SVOData.leaf_voxels gives for a tree; a DAG needs this walk)."""
    lo = [int(v) for v in lo]
    first = [int(v) for v in first]
    out, stack = [], [(0, 0, 0, 0, 0)]
    while stack:
        node, x, y, z, d = stack.pop()
        if node >= len(lo):
            continue
        inner, valid = lo[node] & 0xFF, (lo[node] >> 8) & 0xFF
        for c in range(8):
            if not (valid >> c) & 1:
                continue
            pos = (2 * x + (c & 1), 2 * y + ((c >> 1) & 1), 2 * z + ((c >> 2) & 1))
            if (inner >> c) & 1:
                stack.append((first[node] + bin(inner & ((1 << c) - 1)).count("1"),) + pos + (d + 1,))
            else:
                out.append(pos + (d + 1,))
    return np.array(out, np.int64).reshape(-1, 4)


def list_findings(rows, leaves, ds):
    """The properties of every splat list: pairwise disjoint boxes, each leaf voxel (x, y, z, level) in
    exactly one box, no box deeper than ds."""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    f = []
    if len(rows) and rows[:, 3].max() > ds:
        f.append(f"a box at depth {int(rows[:, 3].max())} > {ds}")
    # disjoint: no box equals another or lies inside one -- no ancestor of a box (itself included) is listed twice
    keys = {}
    for x, y, z, d in rows.tolist():
        keys[(x, y, z, d)] = keys.get((x, y, z, d), 0) + 1
    if any(v > 1 for v in keys.values()):
        f.append("a box listed twice")
    for x, y, z, d in rows.tolist():
        for up in range(1, d):
            if (x >> up, y >> up, z >> up, d - up) in keys:
                f.append(f"box {(x, y, z, d)} lies inside a listed box")
                break
        if len(f) > 5:
            break
    for x, y, z, lv in np.asarray(leaves, np.int64).reshape(-1, 4).tolist():
        # the boxes holding the voxel: its ancestors (itself included); a box below the voxel's level cannot be
        holds = sum(keys.get((x >> up, y >> up, z >> up, lv - up), 0) for up in range(0, lv))
        if holds != 1:
            f.append(f"leaf voxel {(x, y, z, lv)} lies in {holds} boxes")
            if len(f) > 5:
                break
    return f


# ------------------------------------------------------------------ camera
def camera_matrix(c2w, inv_proj, width, height):
    """M (float64): the unnormalised ray direction of continuous pixel coordinates (fx, fy) is M (fx, fy, 1).
    camera_ray: dir = c2w[:3, :3] (inv_proj (u, v, 0, 1)).xyz with u = 2 fx / W - 1, v = 2 fy / H - 1."""
    c2w = np.asarray(c2w, np.float64)
    ip = np.asarray(inv_proj, np.float64)
    cols = np.stack([ip[:3, 0] * 2.0 / width, ip[:3, 1] * 2.0 / height, ip[:3, 3] - ip[:3, 0] - ip[:3, 1]], axis=1)
    return c2w[:3, :3] @ cols


def beam_camera_model(c2w, inv_proj, width, height):
    """{'M', 'minv', 'org', 'plane', 'corners', 'mid'} in float64 ('org' in float32, the render's own), or
    None for a camera the splat refuses: a non-finite c2w, a singular map, or the longest of the centre and
    the four corner directions (one pixel outside the frame) more than 30 times the shortest."""
    c2w32 = np.asarray(c2w, np.float32)
    if not np.all(np.isfinite(c2w32[:3, :4])):
        return None
    with np.errstate(all="ignore"):
        M = camera_matrix(c2w, inv_proj, width, height)
        if not np.all(np.isfinite(M)) or np.linalg.matrix_rank(M) < 3:
            return None
        minv = np.linalg.inv(M)
    v = view_of_matrix(M, width, height)
    if v is None:
        return None
    org = c2w32[:3, 3] * np.float32(1.0 / 32.0) + np.float32(1.5)   # one multiply (exact) and one add, in f32
    return dict(v, M=M, minv=minv, org=org.astype(np.float32))


def view_of_matrix(M, width, height):
    """The frustum of a pixel -> direction map M: {'plane' (unit normals pointing in, through the directions of
    the points one pixel outside the frame's corners), 'corners', 'mid'}, None when too wide."""
    corners = np.array([[-1.0, -1.0], [width + 1.0, -1.0], [width + 1.0, height + 1.0], [-1.0, height + 1.0]])
    D = np.array([M @ np.array([fx, fy, 1.0]) for fx, fy in corners])
    mid = M @ np.array([0.5 * width, 0.5 * height, 1.0])
    lens = np.linalg.norm(np.vstack([D, mid]), axis=1)
    if not lens.min() > 0.0 or lens.max() > 30.0 * lens.min():
        return None
    plane = []
    for j in range(4):
        nrm = np.cross(D[j], D[(j + 1) % 4])
        nrm /= np.linalg.norm(nrm)
        plane.append(nrm if nrm @ mid >= 0.0 else -nrm)
    return {"plane": np.array(plane), "corners": D, "mid": mid}


def axis_bp(F, cx, cy, width, height, org, gen=1):
    """A camera looking along +z with minv = [[F, 0, cx], [0, F, cy], [0, 0, 1]]: fx = F rel_x / rel_z + cx.
    Raw BeamParams (the planes from the same map; the width of the view is not judged)."""
    minv = np.array([[F, 0.0, cx], [0.0, F, cy], [0.0, 0.0, 1.0]])
    M = np.linalg.inv(minv)
    corners = np.array([[-1.0, -1.0], [width + 1.0, -1.0], [width + 1.0, height + 1.0], [-1.0, height + 1.0]])
    D = np.array([M @ np.array([fx, fy, 1.0]) for fx, fy in corners])
    mid = M @ np.array([0.5 * width, 0.5 * height, 1.0])
    plane = []
    for j in range(4):
        nrm = np.cross(D[j], D[(j + 1) % 4])
        nrm /= np.linalg.norm(nrm)
        plane.append(nrm if nrm @ mid >= 0.0 else -nrm)
    return make_bp(width, height, org, minv, plane, gen)


def beam_params(cm, width, height, gen=1):
    """The raw BeamParams fields of a camera model, rounded to f32 as the host rounds them."""
    return make_bp(width, height, cm["org"], cm["minv"], cm["plane"], gen)


def make_bp(width, height, org, minv, plane, gen=1):
    tx, ty, sx, sy = (width + 7) // 8, (height + 7) // 8, (width + 63) // 64, (height + 63) // 64
    return {"width": width, "height": height, "tiles_x": tx, "tiles_y": ty, "super_x": sx, "super_y": sy,
            "super_off": tx * ty, "global_off": tx * ty + sx * sy, "gen": gen,
            "org": np.asarray(org, np.float32).reshape(3), "minv": np.asarray(minv, np.float32).reshape(9),
            "plane": np.asarray(plane, np.float32).reshape(4, 3)}


# ------------------------------------------------------------------ splat
def _rect_tiles(bp, x0, y0, x1, y1):
    """The kernel's clamps of a pixel rectangle: (kind, tx0, ty0, tx1, ty1) per box, kind 0 = no tile,
    1 = at most 32 tiles, 2 = at most 32 super tiles, 3 = the global word."""
    W, H = float(bp["width"]), float(bp["height"])
    vis = (x1 >= 0.0) & (y1 >= 0.0) & (x0 <= W) & (y0 <= H)
    with np.errstate(invalid="ignore"):
        tx0 = np.floor(np.clip(x0, 0.0, 1e9) * 0.125).astype(np.int64)
        ty0 = np.floor(np.clip(y0, 0.0, 1e9) * 0.125).astype(np.int64)
        tx1 = np.minimum(np.floor(np.clip(np.minimum(x1, W), -1e9, 1e9) * 0.125).astype(np.int64), bp["tiles_x"] - 1)
        ty1 = np.minimum(np.floor(np.clip(np.minimum(y1, H), -1e9, 1e9) * 0.125).astype(np.int64), bp["tiles_y"] - 1)
    vis &= (tx1 >= tx0) & (ty1 >= ty0)
    nt = (tx1 - tx0 + 1) * (ty1 - ty0 + 1)
    ns = ((tx1 >> 3) - (tx0 >> 3) + 1) * ((ty1 >> 3) - (ty0 >> 3) + 1)
    kind = np.where(nt <= 32, 1, np.where(ns <= 32, 2, 3))
    kind = np.where(vis, kind, 0)
    return kind, tx0, ty0, tx1, ty1


def _pairs(sel, x0, y0, x1, y1, stride):
    """(box, cell) pairs of the inclusive cell rectangles of the boxes `sel`; cell = y * stride + x."""
    sel = np.asarray(sel, np.int64)
    if len(sel) == 0:
        return sel, sel
    w = (x1[sel] - x0[sel] + 1).astype(np.int64)
    cnt = w * (y1[sel] - y0[sel] + 1)
    which = np.repeat(np.arange(len(sel)), cnt)
    local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    cell = (y0[sel][which] + local // w[which]) * stride + x0[sel][which] + local % w[which]
    return sel[which], cell


class _Levels:
    """A bound per tile, per super tile and for the frame; eff() is the min a reader of the tile takes."""

    def __init__(self, bp):
        self.bp = bp
        self.t = np.full(bp["tiles_x"] * bp["tiles_y"], INF)
        self.s = np.full(bp["super_x"] * bp["super_y"], INF)
        self.g = INF

    def add(self, kind, tx0, ty0, tx1, ty1, d):
        bp = self.bp
        b, cell = _pairs(np.flatnonzero(kind == 1), tx0, ty0, tx1, ty1, bp["tiles_x"])
        np.minimum.at(self.t, cell, d[b])
        b, cell = _pairs(np.flatnonzero(kind == 2), tx0 >> 3, ty0 >> 3, tx1 >> 3, ty1 >> 3, bp["super_x"])
        np.minimum.at(self.s, cell, d[b])
        if np.any(kind == 3):
            self.g = min(self.g, float(d[kind == 3].min()))

    def eff(self):
        bp = self.bp
        ty, tx = np.divmod(np.arange(bp["tiles_x"] * bp["tiles_y"]), bp["tiles_x"])
        return np.minimum(np.minimum(self.t, self.s[(ty >> 3) * bp["super_x"] + (tx >> 3)]), self.g)


_CORNERS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.float64)
_PAIRS28 = np.array([(a, b) for a in range(8) for b in range(a + 1, 8)])


def splat_model(bp, boxes):
    """The envelope of what beam_splat_kernel must leave in a fresh buffer, from the raw BeamParams fields
    (make_bp) and the box words.  Returns a dict: per box d_rule, d_true, cls ('behind' 0, 'at camera' 1,
    'in front' 2, 'straddling' 3), band (in the at-camera band, either kind), amb (ambiguous kind), proj_err;
    per tile hi_rule, lo_rule, hi_geo, geo_box, geo_tol; touched (a tile word some outer rectangle reaches),
    no_claim (a straddling or band box exists: no lower bound anywhere), levels (the highest kind a box can take).

    A straddling box's clipped projection is not modelled: such a box (and one in the at-camera band) takes
    every lower claim of the case away, and enters the upper side through hi_geo alone."""
    rows = box_rows(boxes)
    N = len(rows)
    W, H = bp["width"], bp["height"]
    size = 2.0 ** -rows[:, 3].astype(np.float64)
    lo = 1.0 + rows[:, :3] * size[:, None]                      # exact: 17 significant bits
    org32 = bp["org"].astype(np.float32)
    size32 = size.astype(np.float32)
    rel32 = lo.astype(np.float32) - org32[None, :]              # one IEEE rounding, as in the kernel
    rs32 = rel32 + size32[:, None]
    gap = np.maximum(np.maximum(rel32.astype(np.float64), -rs32.astype(np.float64)), 0.0)
    d_rule = np.sqrt((gap * gap).sum(1))
    org = org32.astype(np.float64)
    rel = lo - org[None, :]                                     # exact in float64
    gap_t = np.maximum(np.maximum(rel, -(rel + size[:, None])), 0.0)
    d_true = np.sqrt((gap_t * gap_t).sum(1))
    minv = bp["minv"].astype(np.float64).reshape(3, 3)
    plane = bp["plane"].astype(np.float64)
    P = rel[:, None, :] + _CORNERS[None, :, :] * size[:, None, None]   # N x 8 x 3
    q = P @ minv.T
    zmin, zmax = q[:, :, 2].min(1), q[:, :, 2].max(1)
    span = np.abs(rel).sum(1) + 3.0 * size
    top = rel @ plane.T + size[:, None] * np.maximum(plane, 0.0).sum(1)[None, :]
    behind = (zmax <= 0.0) | np.any(top < -1e-4 * span[:, None], axis=1)
    at_cam = ~behind & (d_true <= 0.5e-3 * size)
    band = ~behind & ~at_cam & (d_true <= 2e-3 * size)
    front = ~behind & ~at_cam & (zmin > 1e-3 * zmax)
    straddle = ~behind & ~at_cam & ~front
    cls = np.where(behind, 0, np.where(at_cam, 1, np.where(front, 2, 3)))

    # in front: the float64 rectangle of the projected corners, grown by the margin -+ DELTA
    with np.errstate(all="ignore"):
        fx, fy = q[:, :, 0] / q[:, :, 2], q[:, :, 1] / q[:, :, 2]
    x0, x1, y0, y1 = fx.min(1), fx.max(1), fy.min(1), fy.max(1)
    fr = np.flatnonzero(front)
    zero = np.zeros(N, np.int64)
    kin = zero.copy()
    kout = zero.copy()
    ri = [zero.copy() for _ in range(4)]
    ro = [zero.copy() for _ in range(4)]
    if len(fr):
        k, *r = _rect_tiles(bp, x0[fr] - (MG - DELTA), y0[fr] - (MG - DELTA), x1[fr] + (MG - DELTA), y1[fr] + (MG - DELTA))
        kin[fr] = k
        for a, b in zip(ri, r):
            a[fr] = b
        k, *r = _rect_tiles(bp, x0[fr] - (MG + DELTA), y0[fr] - (MG + DELTA), x1[fr] + (MG + DELTA), y1[fr] + (MG + DELTA))
        kout[fr] = k
        for a, b in zip(ro, r):
            a[fr] = b
    amb = front & (kin != kout)
    # the projection's own f32 error (pixels): 16 roundings of 2^-24 on the terms of q's rows; a pixel
    # coordinate that matters lies within the frame, so |f| <= max(W, H) + 1 scales the error of q_z
    S = (np.abs(minv)[None, :, :] * (np.abs(rel) + size[:, None])[:, None, :]).sum(2)   # N x 3
    with np.errstate(all="ignore"):
        proj_err = np.where(front, 16.0 * 2.0 ** -24 * (np.maximum(S[:, 0], S[:, 1]) + (max(W, H) + 1.0) * S[:, 2]) / zmin, 0.0)

    hi, lo_env = _Levels(bp), _Levels(bp)
    # upper: a certain kind at its inner rectangle; an ambiguous box with its inner tiles only; at the camera: global
    up_kind = np.where(amb, np.minimum(kin, 1), kin)
    up_kind = np.where(band, 0, up_kind)          # a band box may be kind 3 instead: its own rule claims nothing
    up_kind = np.where(at_cam, 3, up_kind)
    hi.add(up_kind, *ri, d_rule)
    # lower: the outer rectangle at its (looser) kind; a band box may also be global
    lo_kind = np.where(at_cam | band, 3, kout)
    lo_env.add(lo_kind, *ro, d_rule)
    no_claim = bool(np.any(straddle))
    lo_rule = np.full(len(hi.t), -INF) if no_claim else lo_env.eff()
    # the tile words a kind-1 write can reach: the outer rectangles of the boxes that may be kind 1
    touched = np.zeros(len(hi.t), bool)
    touched[_pairs(np.flatnonzero((kout >= 1) & (kin <= 1) & ~at_cam), *ro, bp["tiles_x"])[1]] = True
    levels = int(lo_kind.max()) if N else 0

    # geometry: the tiles whose rectangle, shrunk by 1e-3 px and cut to the frame, meets the projected box
    T = bp["tiles_x"] * bp["tiles_y"]
    hi_geo = np.full(T, INF)
    geo_box = np.full(T, -1, np.int64)

    def take(b, cell):
        if len(b) == 0:
            return
        order = np.lexsort((b, d_true[b], cell))
        b, cell = b[order], cell[order]
        firsts = np.concatenate([[True], cell[1:] != cell[:-1]])
        b, cell = b[firsts], cell[firsts]
        better = d_true[b] < hi_geo[cell]
        hi_geo[cell[better]] = d_true[b[better]]
        geo_box[cell[better]] = b[better]

    sh = 1e-3
    g = np.flatnonzero(front & (x1 >= 0.0) & (y1 >= 0.0) & (x0 <= W) & (y0 <= H))
    if len(g):
        bx0 = np.floor(np.clip(x0[g], 0.0, W) / 8.0).astype(np.int64)
        by0 = np.floor(np.clip(y0[g], 0.0, H) / 8.0).astype(np.int64)
        bx1 = np.minimum(np.floor(np.clip(x1[g], 0.0, W) / 8.0).astype(np.int64), bp["tiles_x"] - 1)
        by1 = np.minimum(np.floor(np.clip(y1[g], 0.0, H) / 8.0).astype(np.int64), bp["tiles_y"] - 1)
        full = [np.zeros(N, np.int64) for _ in range(4)]
        for a, b in zip(full, (bx0, by0, bx1, by1)):
            a[g] = b
        # separating axes: the frame's own and the normal of every pair of corners (every hull edge is among them)
        slot = np.full(N, -1, np.int64)
        slot[g] = np.arange(len(g))
        pts = np.stack([fx[g], fy[g]], axis=2)                        # boxes x 8 x 2
        e = pts[:, _PAIRS28[:, 1], :] - pts[:, _PAIRS28[:, 0], :]
        nrm = np.stack([-e[:, :, 1], e[:, :, 0]], axis=2)
        nrm = np.concatenate([nrm, np.broadcast_to(np.array([[1.0, 0.0], [0.0, 1.0]]), (len(g), 2, 2))], axis=1)
        proj = np.einsum("nad,npd->nap", nrm, pts)                    # boxes x 30 x 8
        pmin, pmax = proj.min(2), proj.max(2)
        cnt = np.cumsum((bx1 - bx0 + 1) * (by1 - by0 + 1))
        cuts = np.searchsorted(cnt // 100000, np.arange(int(cnt[-1] // 100000) + 2))   # ~100 k pairs at a time
        for c0, c1 in zip(cuts[:-1], cuts[1:]):
            if c1 == c0:
                continue
            b, cell = _pairs(g[c0:c1], *full, bp["tiles_x"])
            cy, cx = np.divmod(cell, bp["tiles_x"])
            rx0, ry0 = cx * 8.0 + sh, cy * 8.0 + sh
            rx1, ry1 = np.minimum(cx * 8.0 + 8.0, W) - sh, np.minimum(cy * 8.0 + 8.0, H) - sh
            mx, my, hx, hy = 0.5 * (rx0 + rx1), 0.5 * (ry0 + ry1), 0.5 * (rx1 - rx0), 0.5 * (ry1 - ry0)
            k = slot[b]
            n_ = nrm[k]                                               # pairs x 30 x 2
            c_ = n_[:, :, 0] * mx[:, None] + n_[:, :, 1] * my[:, None]
            r_ = np.abs(n_[:, :, 0]) * hx[:, None] + np.abs(n_[:, :, 1]) * hy[:, None]
            meets = np.all((c_ + r_ >= pmin[k]) & (c_ - r_ <= pmax[k]), axis=1) & (hx > 0) & (hy > 0)
            take(b[meets], cell[meets])
    # straddling boxes and boxes at the camera: 5^3 witness points in front of the camera plane
    w5 = np.array([[i, j, k] for i in range(5) for j in range(5) for k in range(5)], np.float64) / 4.0
    for i in np.flatnonzero(straddle | at_cam | band):
        qw = (rel[i][None, :] + w5 * size[i]) @ minv.T
        ok = qw[:, 2] > 1e-3 * zmax[i]
        if not ok.any():
            continue
        wx, wy = qw[ok, 0] / qw[ok, 2], qw[ok, 1] / qw[ok, 2]
        inside = (wx > 0) & (wy > 0) & (wx < W) & (wy < H)
        wx, wy = wx[inside], wy[inside]
        cx, cy = np.floor(wx / 8.0).astype(np.int64), np.floor(wy / 8.0).astype(np.int64)
        keep = (wx - 8 * cx > sh) & (wy - 8 * cy > sh) & (wx < np.minimum(8 * cx + 8, W) - sh) & \
               (wy < np.minimum(8 * cy + 8, H) - sh)
        cell = np.unique(cy[keep] * bp["tiles_x"] + cx[keep])
        take(np.full(len(cell), i, np.int64), cell)
    ext = (np.abs(rel32.astype(np.float64)) + size[:, None]).sum(1)
    geo_tol = np.where(geo_box >= 0, 2.0 ** -23 * np.append(ext, 0.0)[geo_box], 0.0)
    return {"d_rule": d_rule, "d_true": d_true, "cls": cls, "band": band, "amb": amb, "proj_err": proj_err,
            "kind_in": kin, "kind_out": kout, "rect_in": ri, "rect_out": ro,
            "hi_rule": hi.eff(), "lo_rule": lo_rule, "hi_geo": hi_geo, "geo_box": geo_box, "geo_tol": geo_tol,
            "touched": touched, "no_claim": no_claim, "levels": levels, "hi_levels": hi, "lo_levels": lo_env}


def case_conditions(m):
    """(share of ambiguous boxes among those in front, pinned share: the touched tiles with hi_rule == lo_rule,
    largest projection error in pixels) of a model."""
    front = m["cls"] == 2
    amb = float(m["amb"].sum()) / max(int(front.sum()), 1)
    touched = np.isfinite(m["lo_rule"]) | np.isfinite(m["hi_rule"])
    pinned = float(np.sum(m["hi_rule"][touched] == m["lo_rule"][touched])) / max(int(touched.sum()), 1)
    return amb, pinned, float(m["proj_err"].max()) if len(m["proj_err"]) else 0.0


# ------------------------------------------------------------------ the buffer
def decode(words64, bp, gen):
    """(E per tile, tile / super / global distances) of a buffer of u64 keys read at generation `gen`: an
    entry whose high half is ~gen holds its distance, any other reads as +inf."""
    w = np.asarray(words64, np.uint64)
    hi = (w >> np.uint64(32)).astype(np.uint32)
    d = (w & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32).astype(np.float64)
    d = np.where(hi == np.uint32(~gen & 0xFFFFFFFF), d, INF)
    lv = _Levels(bp)
    lv.t, lv.s, lv.g = d[:bp["super_off"]], d[bp["super_off"]:bp["global_off"]], float(d[bp["global_off"]])
    return lv.eff(), lv


def buffer_words(bp):
    return bp["global_off"] + 1


def check_envelope(E, m):
    """The three per-tile properties; a list of findings."""
    f = []
    safe = m["hi_geo"] * (1.0 + REL) + m["geo_tol"]
    bad = np.flatnonzero(E > safe)
    if len(bad):
        f.append(f"safety: {len(bad)} tiles above the geometric bound, first tile {int(bad[0])}: "
                 f"E = {E[bad[0]]!r} > {safe[bad[0]]!r} (box {int(m['geo_box'][bad[0]])})")
    bad = np.flatnonzero(E > m["hi_rule"] * (1.0 + REL))
    if len(bad):
        f.append(f"rule, upper: {len(bad)} tiles, first tile {int(bad[0])}: E = {E[bad[0]]!r} > {m['hi_rule'][bad[0]]!r}")
    with np.errstate(invalid="ignore"):
        low = np.where(np.isfinite(m["lo_rule"]), m["lo_rule"] * (1.0 - REL), m["lo_rule"])
    bad = np.flatnonzero(E < low)
    if len(bad):
        f.append(f"rule, lower: {len(bad)} tiles, first tile {int(bad[0])}: E = {E[bad[0]]!r} < {m['lo_rule'][bad[0]]!r}")
    return f


def check_structure(words32, bp, gen, m=None):
    """Exact, for a buffer that was all-ones before the launch: the guard words, every high half ~gen or
    all-ones; with a model that makes lower claims, the words no box can reach."""
    f = []
    n = buffer_words(bp)
    w = np.asarray(words32, np.uint32)
    if len(w) != 2 * n + GUARD_WORDS:
        return [f"{len(w)} words, not {2 * n} + {GUARD_WORDS}"]
    if np.any(w[2 * n:] != GUARD):
        f.append("a guard word overwritten")
    w64 = w[:2 * n].view(np.uint64)
    hi = (w64 >> np.uint64(32)).astype(np.uint32)
    ones = w64 == np.uint64(0xFFFFFFFFFFFFFFFF)
    if np.any(~ones & (hi != np.uint32(~gen & 0xFFFFFFFF))):
        f.append("a word whose high half is neither ~gen nor all-ones")
    if m is not None and not m["no_claim"]:
        if np.any(~ones[:bp["super_off"]] & ~m["touched"]):
            f.append("a tile word outside every outer rectangle was written")
        if m["levels"] < 2 and np.any(~ones[bp["super_off"]:bp["global_off"]]):
            f.append("a super tile word written without a box above 32 tiles")
        if m["levels"] < 3 and not ones[bp["global_off"]]:
            f.append("the global word written without a box above 32 super tiles")
    return f


# ------------------------------------------------------------------ tests/beam_splat_driver.cpp's files
def write_cases(path, cases):
    """cases: dicts {'bp': make_bp(...), 'boxes': words (N x 2), 'steps': [(gen, bp of that step)]}."""
    out = [np.array([MAGIC, len(cases)], np.uint32)]
    for c in cases:
        bp = c["bp"]
        boxes = np.ascontiguousarray(c["boxes"], np.uint32).reshape(-1, 2)
        out.append(np.array([bp[k] for k in ("width", "height", "tiles_x", "tiles_y", "super_x", "super_y", "super_off",
                                             "global_off")] + [len(boxes), len(c["steps"])], np.uint32))
        out.append(boxes.reshape(-1))
        for gen, sbp in c["steps"]:
            out.append(np.array([gen], np.uint32))
            out.append(np.concatenate([sbp["org"], sbp["minv"], sbp["plane"].reshape(-1)]).astype(np.float32).view(np.uint32))
    np.concatenate(out).astype("<u4").tofile(path)


def read_results(path, cases):
    """Per case the list of buffers (u32 words, guard words included), one after each step."""
    w = np.fromfile(path, "<u4")
    assert w[0] == MAGIC and w[1] == len(cases), "result file: bad header"
    at, out = 2, []
    for c in cases:
        assert int(w[at]) == len(c["steps"]), "result file: step count"
        at += 1
        bufs = []
        for _ in c["steps"]:
            err, ln = int(w[at]), int(w[at + 1])
            assert err == 0, f"hipError {err}"
            bufs.append(w[at + 2:at + 2 + ln])
            at += 2 + ln
        out.append(bufs)
    assert at == len(w), "result file: trailing words"
    return out
