"""The mesh rule in numpy (csrc/svo_voxelize.h restated term for term, float32, one rounding per operation):
which voxels of the 2^depth grid a triangle mesh makes surface leaves, which triangle owns each leaf, and the
leaf's normal and colour.  svob_mesh_leaves / svob_build_mesh (native_builder.mesh_leaves / build_mesh_svo)
compute the same on the GPU, bit for bit.

  voxelize(positions, triangles, depth, colors=None, flip=False) -> (codes, normals, colors_or_None, owner)
  fit_mesh(positions, margin) -> positions mapped uniformly into the unit cube (not part of the rule)

Positions are in the cube's unit frame [0,1]^3 (the tracer's [1,2]^3); grid coordinates are p * 2^depth."""
import numpy as np

from .builder import morton, normalize_unity

F = np.float32
NO_OWNER = np.uint32(0xFFFFFFFF)


def _cross(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


def _dot(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


class Tri:
    """svo_voxelize::Tri of one triangle: `setup` of the header."""

    def __init__(self, p, n):
        fn = F(n)
        self.v = v = (np.asarray(p, F).reshape(3, 3) * fn).astype(F)
        a = [v[1, c] - v[0, c] for c in range(3)]
        b = [v[2, c] - v[0, c] for c in range(3)]
        self.a3, self.b3 = a, b
        self.n = N = [F(x) for x in _cross(a, b)]
        self.w = (abs(N[0]) + abs(N[1])) + abs(N[2])
        with np.errstate(all="ignore"):
            self.unit = normalize_unity(np.array([N], F))[0]
        self.degenerate = bool(np.all(self.unit == 0))
        self.blo, self.bhi = [], []
        for c in range(3):
            mn, mx = v[0, c], v[0, c]
            for k in (1, 2):
                mn = v[k, c] if v[k, c] < mn else mn
                mx = v[k, c] if v[k, c] > mx else mx
            self.blo.append(0 if mn <= 0 else n if mn > fn else int(np.ceil(mn)) - 1)
            self.bhi.append(-1 if mx < 0 else n - 1 if mx >= fn else int(np.floor(mx)))
        self.outside = any(lo > hi for lo, hi in zip(self.blo, self.bhi))
        self.edges = []   # [projection][edge] (u, v, e, A_u, A_v, lo, hiw)
        with np.errstate(all="ignore"):
            for q in range(3):
                u, w = q, (q + 1) % 3
                for e in range(3):
                    f, g = (e + 1) % 3, (e + 2) % 3
                    au = -(v[f, w] - v[e, w])
                    av = v[f, u] - v[e, u]
                    t = au * (v[g, u] - v[e, u]) + av * (v[g, w] - v[e, w])
                    lo = t if t < 0 else F(0)
                    hiw = (t if t > 0 else F(0)) + (abs(au) + abs(av))
                    self.edges.append((u, w, e, F(au), F(av), F(lo), F(hiw)))

    @property
    def skipped(self):
        return self.degenerate or self.outside

    def candidates(self):
        if self.skipped:
            return 0
        return int(np.prod([hi - lo + 1 for lo, hi in zip(self.blo, self.bhi)]))

    def overlaps(self):
        """Steps 2 and 3 for every voxel of the box: a bool array [z, y, x] over the box."""
        ax = [np.arange(self.blo[c], self.bhi[c] + 1, dtype=np.int64) for c in range(3)]
        shape = [(1, 1, -1), (1, -1, 1), (-1, 1, 1)]
        lo = [ax[c].astype(F).reshape(shape[c]) for c in range(3)]
        hi = [(ax[c] + 1).astype(F).reshape(shape[c]) for c in range(3)]
        return np.broadcast_to(self._rule(lo, hi), (len(ax[2]), len(ax[1]), len(ax[0])))

    def overlaps_at(self, ijk):
        """Steps 2 and 3 for the listed voxels ijk [m, 3] (integers inside the box): bool [m].  The header allows
        any pruning of candidates; this is `overlaps` on a caller's selection of them."""
        ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
        return self._rule([ijk[:, c].astype(F) for c in range(3)], [(ijk[:, c] + 1).astype(F) for c in range(3)])

    def _rule(self, lo, hi):
        """lo, hi: per axis the voxels' lower and upper faces as float32 arrays that broadcast together."""
        v, N = self.v, self.n
        with np.errstate(all="ignore"):
            d = [(hi[c] if N[c] > 0 else lo[c]) - v[0, c] for c in range(3)]
            s = (N[0] * d[0] + N[1] * d[1]) + N[2] * d[2]
            ok = (s >= 0) & (s <= self.w)
            for u, w, e, au, av, elo, hiw in self.edges:
                p = au * ((hi[u] if au > 0 else lo[u]) - v[e, u]) + av * ((hi[w] if av > 0 else lo[w]) - v[e, w])
                ok = ok & (p >= elo) & (p <= hiw)
        return ok

    def normal(self, flip=False):
        return (-self.unit if flip else self.unit).astype(F)

    def color(self, ijk, c0, c1, c2):
        """leaf_color for voxels ijk [m, 3] (integers) and the owner's vertex colours."""
        ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
        a, b, N = self.a3, self.b3, self.n
        with np.errstate(all="ignore"):
            q = [(ijk[:, c].astype(F) + F(0.5)) - self.v[0, c] for c in range(3)]
            d = _dot(N, N)
            w1 = _dot(_cross(q, b), N) / d
            w2 = _dot(_cross(a, q), N) / d
            w0 = (F(1) - w1) - w2
            w0, w1, w2 = [np.where(w > 0, w, F(0)).astype(F) for w in (w0, w1, w2)]
            s = (w0 + w1) + w2
            w0, w1, w2 = w0 / s, w1 / s, w2 / s
            c0, c1, c2 = [np.asarray(c, F) for c in (c0, c1, c2)]
            return np.stack([(w0 * c0[c] + w1 * c1[c]) + w2 * c2[c] for c in range(3)], axis=1).astype(F)


def _check_mesh(positions, triangles, colors):
    pos = np.ascontiguousarray(positions, F).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles, np.int64).reshape(-1, 3)
    if not np.all(np.isfinite(pos)):
        raise ValueError("positions must be finite")
    if tri.size and (tri.min() < 0 or tri.max() >= len(pos)):
        raise ValueError("a triangle index is outside the vertices")
    col = None
    if colors is not None:
        col = np.ascontiguousarray(colors, F).reshape(-1, 3)
        if len(col) != len(pos):
            raise ValueError("colors must hold one rgb per vertex")
    return pos, tri, col


def setup(positions, triangles, depth):
    """The per-triangle constants of a mesh: a list of Tri."""
    pos, tri, _ = _check_mesh(positions, triangles, None)
    return [Tri(pos[t], 1 << depth) for t in tri]


def owner_grid(tris, depth):
    """(owner [z, y, x] uint32 with NO_OWNER where no triangle passes, stats dict)."""
    n = 1 << depth
    grid = np.full((n, n, n), NO_OWNER, np.uint32)
    stats = {"degenerate": 0, "outside": 0, "candidates": 0, "overlaps": 0}
    for k, t in enumerate(tris):
        if t.degenerate:
            stats["degenerate"] += 1
            continue
        if t.outside:
            stats["outside"] += 1
            continue
        ok = t.overlaps()
        stats["candidates"] += t.candidates()
        stats["overlaps"] += int(ok.sum())
        sl = tuple(slice(t.blo[c], t.bhi[c] + 1) for c in (2, 1, 0))
        sub = grid[sl]
        grid[sl] = np.where(ok, np.minimum(sub, np.uint32(k)), sub)
    return grid, stats


def voxelize(positions, triangles, depth, colors=None, flip=False, want_stats=False):
    """(codes uint64 [m] sorted unique Morton codes (x bit 0, y bit 1, z bit 2), normals f32 [m, 3],
    colors f32 [m, 3] or None, owner uint32 [m]); with want_stats a fifth item, the dict of
    svob_mesh_stats' counts."""
    pos, tri, col = _check_mesh(positions, triangles, colors)
    if not 1 <= depth <= 21:
        raise ValueError("depth must be in [1, 21]")
    tris = [Tri(pos[t], 1 << depth) for t in tri]
    grid, stats = owner_grid(tris, depth)
    z, y, x = np.nonzero(grid != NO_OWNER)
    xyz = np.stack([x, y, z], axis=1).astype(np.uint32)
    codes = morton(xyz) if len(xyz) else np.zeros(0, np.uint64)
    order = np.argsort(codes, kind="stable")
    codes, xyz = codes[order].astype(np.uint64), xyz[order]
    owner = grid[xyz[:, 2], xyz[:, 1], xyz[:, 0]].astype(np.uint32)
    normals = np.zeros((len(codes), 3), F)
    out_col = None if col is None else np.zeros((len(codes), 3), F)
    for k in np.unique(owner):
        at = np.flatnonzero(owner == k)
        normals[at] = tris[k].normal(flip)
        if col is not None:
            i0, i1, i2 = tri[k]
            out_col[at] = tris[k].color(xyz[at], col[i0], col[i1], col[i2])
    out = (codes, normals, out_col, owner)
    return out + (stats,) if want_stats else out


def leaf_xyz(codes):
    """Integer voxel coordinates [m, 3] of Morton codes."""
    codes = np.asarray(codes, np.uint64)
    out = np.zeros((len(codes), 3), np.uint32)
    for bit in range(21):
        for c in range(3):
            out[:, c] |= (((codes >> np.uint64(3 * bit + c)) & np.uint64(1)) << np.uint64(bit)).astype(np.uint32)
    return out


def fit_mesh(positions, margin=0.05):
    """Map a mesh's bounding box uniformly (one scale, centred) into [margin, 1 - margin]^3.  A convenience in
    float64, rounded once to float32; not part of the bit-exact rule."""
    p = np.asarray(positions, np.float64).reshape(-1, 3)
    if not 0 <= margin < 0.5:
        raise ValueError("margin must lie in [0, 0.5)")
    if len(p) == 0:
        return p.astype(F)
    lo, hi = p.min(0), p.max(0)
    extent = float((hi - lo).max())
    scale = (1.0 - 2.0 * margin) / extent if extent > 0 else 1.0
    return (0.5 + (p - (lo + hi) / 2) * scale).astype(F)
