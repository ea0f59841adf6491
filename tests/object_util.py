"""Shared helpers of the scene-object tests (tests/test_objects.py, tests/test_gpu_objects.py): the pool (tree7 as
the terrain at offset 0, the Text fixture and a second tree7 behind it, all v1 uploads), the committed
placements, and the expected records of svo_trace_scene and of a render with svo_set_objects, built from the
CPU oracle and numpy alone.

Nothing is extracted or re-uploaded for the expectation: each object's OWN tree is traced stand-alone with
reflect_util.oracle_trace on objects.object_rays(...) after query.sanitize_rays, `root` is added to `parent`,
and objects.cube_test, query.apply_t_max, objects.world_normal and objects.fold_nearest do the rest.  The
terrain candidate is the oracle's record of the world ray; colours come from reflect_util.shade_hit."""
import numpy as np

from raytracingtest_amd import objects as rule
from raytracingtest_amd import sky as sky_rule
from raytracingtest_amd.camera import main_camera, main_light
from raytracingtest_amd.query import apply_t_max, camera_rays, sanitize_rays
from tests import query_util as qu
from tests import reflect_util as ru
from tests.query_util import MISS, pack_mask

f32 = np.float32


def rot(axis, deg):
    """Rotation by `deg` degrees about a unit axis (Rodrigues), float64 3 x 3."""
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def axis_rotations():
    """The 24 proper rotations that map the axes onto the axes (entries 0, +-1)."""
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for signs in range(8):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = -1.0 if (signs >> i) & 1 else 1.0
            if np.linalg.det(R) > 0:
                out.append(R)
    assert len(out) == 24
    return out


class Scene:
    """The suite's pool: `uploads` [(SVOData, offset)] in order, `trees` {name: (SVOData, root)}."""

    def __init__(self, both):
        tree7, text = both["tree7"], both["text"]
        assert tree7.format == 1 and text.format == 1
        self.terrain = tree7
        self.trees = {"text": (text, len(tree7)), "tree7b": (tree7, len(tree7) + len(text))}
        self.uploads = [(tree7, 0), (text, self.trees["text"][1]), (tree7, self.trees["tree7b"][1])]
        self.n_nodes = 2 * len(tree7) + len(text)

    def tree_of_root(self, root):
        if root == 0:
            return self.terrain
        for svo, r in self.trees.values():
            if r == root:
                return svo
        raise KeyError(root)

    def upload(self, master):
        for svo, off in self.uploads:
            master.SetSVOBuffer(svo, off)


def placements(scene):
    """The committed placements, by name: (root, scale_log2, position, rotation).  tree7 / Main: the camera
    sits at (1, 1, 1) inside the terrain's cube and looks along +z."""
    text, tree = scene.trees["text"][1], scene.trees["tree7b"][1]
    return {
        "near": (text, -3, (0.0, 1.5, 4.5), rot((0.0, 1.0, 0.0), 30.0)),            # a 4-unit Text cube before the camera
        "far": (tree, -1, (6.0, 3.0, 14.0), rot((1.0, 2.0, 0.5), 40.0)),              # a 16-unit tree among the terrain's voxels
        "behind_near": (tree, -3, (-0.5, 1.25, 7.5), rot((0.0, 0.0, 1.0), 90.0)),   # behind "near" for many pixels
        "low": (text, -1, (-1.0, -7.0, 15.0), np.eye(3)),
        "side": (text, 0, (20.0, 1.0, 24.0), rot((0.3, 1.0, 0.2), 85.0)),             # a 32-unit cube, an edge toward the camera
        "big": (text, 0, (0.0, 0.0, 60.0), rot((0.0, 1.0, 0.0), 180.0)),              # a 32-unit cube far behind everything
        "tiny": (tree, -6, (1.5, 0.9, 2.5), rot((1.0, 1.0, 1.0), 120.0)),            # an axis rotation, a half-unit cube
        "down": (text, -2, (4.0, -5.0, 7.0), rot((0.0, 1.0, 0.0), -60.0)),
    }


ORDER = ("near", "far", "behind_near", "low", "side", "big", "tiny", "down")
SETS = {"one": ORDER[:1], "two": ORDER[:2], "eight": ORDER}


def object_set(scene, name):
    p = placements(scene)
    return rule.make_objects([p[k] for k in SETS[name]])


_cache = {}


def _osvo(oracle_mod, svo):
    key = ("osvo", id(svo))
    if key not in _cache:
        _cache[key] = (ru.oracle_svo(oracle_mod, svo), svo)   # the tree is kept alive with its oracle copy
    return _cache[key][0]


def fold_objects(oracle_mod, tree_of_root, rays, objects, mode, raw, best, ids, pos, vox, alb, invalid_w):
    """Steps 2-6 for objects 0 .. n - 1 on top of (best, ids, pos, vox, alb), all modified in place but `best`
    and `ids`, which are returned.  tree_of_root: root -> the object's own tree (an SVOData, or an oracle SVO).
    Returns (best, ids, stats): stats[j] = masks `go` (walked), `no_cube` (the span test fails), `entry_skip`
    (the span holds and t_entry alone skips the object), `taken`, `replaced` (taken from an earlier object),
    `hit_behind` (walked and hit, but not nearer than the best)."""
    stats = []
    for j, ob in enumerate(objects):
        orays = rule.object_rays(rays, ob)
        traced, invalid_o = sanitize_rays(orays, raw=raw)
        live = ~invalid_w & ~invalid_o
        best_hit = (best["flags"] & 1) != 0
        span = live & rule.cube_test(traced)
        go = live & rule.cube_test(traced, best_hit, best["t"])
        idx = np.flatnonzero(go)
        tree = tree_of_root(int(ob["root"]))
        osvo = tree if hasattr(tree, "s") else _osvo(oracle_mod, tree)
        cand = np.repeat(MISS, len(rays))
        c_alb = np.zeros((len(rays), 3), f32)
        c_vox = np.full(len(rays), ~np.uint64(0), np.uint64)
        if len(idx):
            cand[idx], c_alb[idx], c_vox[idx] = ru.oracle_trace(oracle_mod, osvo, traced[idx], mode)
        hit = (cand["flags"] & 1) != 0
        cand["parent"][hit] += np.uint32(ob["root"])
        keep = apply_t_max(cand, traced["t_max"])
        cand[~keep] = MISS[0]
        cand = rule.world_normal(cand, ob)
        was_object = ids > 0
        taken, best, ids = rule.fold_nearest(best, ids, cand, j + 1, walked=go)
        at = np.flatnonzero(taken)
        if len(at):
            _, p, _ = qu.oracle_trace(oracle_mod, osvo, traced[at], mode)   # the object-local hit position
            pos[at], vox[at], alb[at] = p, c_vox[at], c_alb[at]
        stats.append({"go": go, "no_cube": live & ~span, "entry_skip": span & ~go, "taken": taken,
                      "replaced": taken & was_object, "hit_behind": ((cand["flags"] & 1) != 0) & go & ~taken})
    return best, ids, stats


def scene_expected(oracle_mod, scene, rays, objects, mode=0, raw=False, terrain=True, tree_of_root=None):
    """What svo_trace_scene must write for `rays`: a dict hits / position / voxel / hitmask / object, plus
    `stats` (fold_objects)."""
    objects = rule.make_objects(objects)
    n = len(rays)
    _, invalid_w = sanitize_rays(rays, raw=raw)
    if terrain:
        exp = qu.expected(oracle_mod, _osvo(oracle_mod, scene.terrain), rays, mode, raw)
        best, pos, vox = exp["hits"].copy(), exp["position"].copy(), exp["voxel"].copy()
    else:
        best, pos, vox = np.repeat(MISS, n), np.zeros((n, 4), f32), np.full(n, ~np.uint64(0), np.uint64)
    ids = np.where((best["flags"] & 1) != 0, 0, -1).astype(np.int32)
    alb = np.zeros((n, 3), f32)
    best, ids, stats = fold_objects(oracle_mod, tree_of_root or scene.tree_of_root, rays, objects, mode, raw, best, ids,
                                    pos, vox, alb, invalid_w)
    return {"hits": best, "position": pos, "voxel": vox, "hitmask": pack_mask((best["flags"] & 1) != 0), "object": ids,
            "stats": stats}


def tile_masks(hit, w, h):
    """svo_frame.hitmask of a whole frame: per 8 x 8 tile (ty * tiles_x + tx) the ballot of its hit pixels,
    bit (y % 8) * 8 + x % 8; pixels outside the frame: 0."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    grid = np.zeros((ty * 8, tx * 8), np.uint64)
    grid[:h, :w] = np.asarray(hit, bool).reshape(h, w)
    g = grid.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty, tx, 64)
    return (g << np.arange(64, dtype=np.uint64)[None, None, :]).sum(axis=2, dtype=np.uint64).reshape(-1)


def frame_expected(oracle_mod, scene, objects, w, h, mode=0, off=(0.5, 0.5), texture=None):
    """Every output of a render of tree7 / Main with svo_set_objects(objects): a dict hits / rgba / position /
    voxel / hitmask (numpy, frame order) plus `ids`, `prim` (reflect_util.primary) and `stats`.  texture: None,
    or (texels, bilinear, clamp_v) of svo_set_skybox -- the pixels that stay misses take sky.sample_sky."""
    from tests.ambient_util import camera_dirs
    objects = rule.make_objects(objects)
    prim = ru.primary(oracle_mod, "tree7", scene.terrain, "main", w, h, mode, off)
    c2w, inv_proj = main_camera().uniforms(w, h)
    rays = camera_rays(c2w, inv_proj, w, h, off)
    assert rays[prim["px"]].tobytes() == prim["rays"].tobytes()   # numpy's camera rays are the oracle's
    _, invalid_w = sanitize_rays(rays, raw=True)
    best, pos, vox = prim["hits"].copy(), prim["position"].copy(), prim["voxel"].copy()
    rgba = prim["rgba"].copy()
    ids = np.where((best["flags"] & 1) != 0, 0, -1).astype(np.int32)
    alb = np.zeros((w * h, 3), f32)
    best, ids, stats = fold_objects(oracle_mod, scene.tree_of_root, rays, objects, mode, True, best, ids, pos, vox, alb,
                                    invalid_w)
    at = np.flatnonzero(ids > 0)
    n = np.stack([best["nx"][at], best["ny"][at], best["nz"][at]], axis=1)
    rgba[at, :3] = ru.shade_hit(n, alb[at], main_light())
    rgba[at, 3] = 1.0
    if texture is not None:
        miss = np.flatnonzero((best["flags"] & 1) == 0)
        rgba[miss, :3] = sky_rule.sample_sky(camera_dirs(oracle_mod, "main", w, h, miss, off), *texture)
        rgba[miss, 3] = 1.0
    return {"hits": best, "rgba": rgba, "position": pos, "voxel": vox,
            "hitmask": tile_masks((best["flags"] & 1) != 0, w, h), "ids": ids, "prim": prim, "stats": stats}


def frame_bytes(oracle_mod, exp):
    """frame_expected's outputs as the byte arrays of a svo_render_frame with every output."""
    words = oracle_mod.pack_rgba8(exp["rgba"])
    return {"hits": exp["hits"], "rgba": exp["rgba"], "rgba8": words,
            "compact": np.ascontiguousarray(exp["hits"].view(np.uint32).reshape(-1, 6)[:, :3]),
            "position": exp["position"], "voxel": exp["voxel"],
            "rgb8": np.ascontiguousarray(words.view(np.uint8).reshape(-1, 4)[:, :3]), "hitmask": exp["hitmask"]}


# the non-degeneracy conditions of the "eight" set on tree7 / Main, per frame size: pixel counts (1 % of the
# frame at 200 x 120, a fifth of that share at 64 x 40)
CONDITIONS = {(200, 120): 240, (64, 40): 5}


def classes(exp, w, h):
    """Pixel counts of the classes the pass has a path for, from frame_expected's result."""
    prim_hit = (exp["prim"]["hits"]["flags"] & 1) != 0
    ids, stats = exp["ids"], exp["stats"]
    any_go = np.any([s["go"] for s in stats], axis=0)
    # an object behind the terrain: it was walked and hit, and the primary record stayed
    behind = np.any([s["hit_behind"] for s in stats], axis=0) & prim_hit & (ids == 0)
    tiles = tile_masks(any_go, w, h)   # a tile without a bit: its wave walks no object
    return {
        "in_front": int((prim_hit & (ids > 0)).sum()),
        "behind": int(behind.sum()),
        "over_sky": int((~prim_hit & (ids > 0)).sum()),
        "replaced": int(np.any([s["replaced"] for s in stats], axis=0).sum()),
        "entry_skip": int(np.any([s["entry_skip"] for s in stats], axis=0).sum()),
        "no_cube": int(np.any([s["no_cube"] for s in stats], axis=0).sum()),
        "untouched_tiles": int((tiles == 0).sum()),
    }
