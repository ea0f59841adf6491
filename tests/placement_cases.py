"""The inputs of the placement-kernel tests (tests/test_gpu_placement.py runs them on the GPU,
tests/test_placement_model.py checks on the CPU that they reach what they are meant to reach):
the smallest shapes and the cost patterns at which the order kernels can still go wrong, and the
ray batches of the query keys.  Everything is seeded; building the list takes milliseconds."""
import numpy as np

from raytracingtest_amd.query import make_rays
from tests import placement_model as pm
from tests.query_util import axis_aligned_batch, mixed_batch, random_batch

# thread partly valid (32 costs per thread), wave edge, one chunk of 1024 x 32 exactly (registers kept
# across the passes), a second chunk with one valid element, three chunks
TILE_N = [1, 31, 32, 33, 63, 64, 65, 2047, 32767, 32768, 32769, 70001]
# (240, 135): 1080p, the walk's carry with dc = 7, dr = 79; (8, 1024): dr = 0; (8, 1500): dc = 0
STRIP_SHAPES = [(8, 1), (8, 3), (16, 5), (64, 17), (240, 135), (8, 1024), (8, 1500), (960, 2)]
SEG_CONFIGS = [(0, 0), (1, 0x4), (3, 0x444), (96, 0x888), (5, 0x448), (2, 0x444444)]
QUERY_N = [1, 63, 64, 65, 256, 257, 4133]
THRESHOLDS = [(7, 8), (3, 4), (1, 2), (1, 4), (1, 8)]


def ladder(mx):
    """mx, and for every class threshold p/q the smallest cost on it and the cost just below."""
    out = [mx]
    for p, q in THRESHOLDS:
        on = -(-p * mx // q)
        out += [on, on - 1]
    return np.array(out, np.uint16)


def heavy(rng, n):
    """Heavy-tailed: log-uniform over 13 octaves, so every class down to 1/8 of the max is populated."""
    return np.floor(2.0 ** rng.uniform(0.0, 13.0, n)).astype(np.uint16)


def pattern(name, n, rng):
    if name == "heavy":
        return heavy(rng, n)
    if name == "zero":
        return np.zeros(n, np.uint16)
    if name == "equal":
        return np.full(n, 77, np.uint16)
    if name == "single":
        c = np.full(n, 3, np.uint16)
        c[rng.integers(n)] = 5000
        return c
    if name in ("ladder4096", "ladder4095"):
        return rng.permutation(np.resize(ladder(int(name[6:])), n))
    if name == "top":
        c = heavy(rng, n)
        c[rng.integers(n)] = 0x7FFF
        return c
    if name == "bit15":   # the tile order's mask must drop it
        c = heavy(rng, n)
        c[rng.random(n) < 0.5] |= 0x8000
        return c
    raise ValueError(name)


def strip_pattern(name, tiles_x, tiles_y, rng):
    """The ladders per XCD (each XCD classes against its own max): XCD x's e-th tile takes rung e."""
    n = tiles_x * tiles_y
    if not name.startswith("ladder"):
        return pattern(name, n, rng)
    lad = ladder(int(name[6:]))
    c = np.zeros((tiles_y, tiles_x), np.uint16)
    for x in range(8):
        own = c[:, x::8]
        c[:, x::8] = np.concatenate([lad[:1], np.resize(np.roll(lad[1:], x), own.size - 1)]).reshape(own.shape)
    return c.reshape(-1)


def flagged(cost, rng):
    """A tenth of the tiles (at least two) become segmented ones: word = SEG_COST_FLAG | 4 or | 8, their
    cost in part_cost (4 or 8 entries); every unused part_cost slot is 0xFFFF."""
    n = len(cost)
    cost = cost.copy()
    part = np.full((n, pm.SEG_KMAX), 0xFFFF, np.uint16)
    pick = rng.permutation(n)[:max(2, n // 10)]
    for i, t in enumerate(pick):
        k = 4 if i % 2 == 0 else 8
        cost[t] = pm.SEG_COST_FLAG | k
        part[t, :k] = heavy(rng, k)
    return cost, part.reshape(-1)


def tile_cases():
    rng = np.random.default_rng(101)
    cases = []
    for n in TILE_N:
        for name in ("heavy", "zero", "equal", "single", "ladder4096", "ladder4095", "top", "bit15"):
            cases.append((f"tiles n={n} {name}", pm.case_tiles(pattern(name, n, rng), n)))
    cases.append(("tiles n=2047 heavy, no stats", pm.case_tiles(heavy(rng, 2047), 2047, with_stats=False)))
    return cases


def repeat_cases():
    """The tile order has no atomics: the same case twice must give identical bytes."""
    rng = np.random.default_rng(103)
    out = []
    for n in (2047, 70001):
        c = heavy(rng, n)
        out += [(f"tiles n={n} repeat {i}", pm.case_tiles(c, n)) for i in range(2)]
    return out


def strip_cases():
    rng = np.random.default_rng(107)
    cases = []
    for tx, ty in STRIP_SHAPES:
        n = tx * ty
        for cap, kpack in SEG_CONFIGS:
            for spread in (0, 1):
                cost, part = heavy(rng, n), None
                if cap:
                    cost, part = flagged(cost, rng)
                cases.append((f"strips {tx}x{ty} cap={cap} kpack={kpack:#x} spread={spread} heavy",
                              pm.case_strips(cost, n, tx, cap, kpack, spread, part)))
        for cap, kpack in ((0, 0), (1, 0x4), (3, 0x444), (5, 0x448)):
            for name in ("zero", "equal", "single", "ladder4096", "ladder4095", "top"):
                for spread in ((0, 1) if name.startswith("ladder") else (0,)):
                    cases.append((f"strips {tx}x{ty} cap={cap} kpack={kpack:#x} spread={spread} {name}",
                                  pm.case_strips(strip_pattern(name, tx, ty, rng), n, tx, cap, kpack, spread)))
    # flagged words with part_cost null: the word's low 15 bits are the cost
    for tx, ty in ((16, 5), (240, 135)):
        cost, _ = flagged(heavy(rng, tx * ty), rng)
        cases.append((f"strips {tx}x{ty} flagged, part_cost null", pm.case_strips(cost, tx * ty, tx, 3, 0x444, 0, None)))
    cases.append(("strips 64x17 no stats", pm.case_strips(heavy(rng, 64 * 17), 64 * 17, 64, 3, 0x444, 0, None,
                                                          with_stats=False)))
    return cases


def refusal_cases():
    c = np.full(64, 9, np.uint16)
    return [("refuse kpack nibble 3", pm.case_strips(c, 64, 8, 1, 0x3)),
            ("refuse kpack nibble 15 in class 5, no seg_cap", pm.case_strips(c, 64, 8, 0, 0xF00000)),
            ("refuse n no multiple of tiles_x", pm.case_strips(c[:24], 24, 16, 1, 0x4)),
            ("refuse grid of 2^28 exactly", pm.case_strips(c, 64, 8, 11184808, 0x4))]


def special_rays():
    """Origins exactly on each face, edge and corner of the cube [-16, 16]^3, origins inside it
    (t_min = 0: the entry point is the origin) and rays whose entry cell is 0 or 511 on some axis."""
    rng = np.random.default_rng(109)
    o, d = [], []
    inner = (-3.7, 5.3, 11.9)
    for ix in range(3):
        for iy in range(3):
            for iz in range(3):
                if ix == iy == iz == 1:
                    continue
                p = np.array([(-16.0, inner[0], 16.0)[ix], (-16.0, inner[1], 16.0)[iy], (-16.0, inner[2], 16.0)[iz]])
                dirs = [-p, p, (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0)] + list(rng.normal(size=(3, 3)))
                o += [p] * len(dirs)
                d += dirs
    for _ in range(64):   # inside
        o.append(rng.uniform(-15.9, 15.9, 3))
        d.append(rng.normal(size=3))
    edge = (-16.0, -15.99, -15.9376, 15.9374, 15.99, 15.999999, 16.0)   # cells 0, 0, 0 (just below 1), 510 (just below 511), 511, 511, 511 (the far face, clamped)
    for a in range(3):
        for sgn in (1.0, -1.0):
            for u in edge:
                for v in edge:
                    p = np.zeros(3)
                    p[a], p[(a + 1) % 3], p[(a + 2) % 3] = -40.0 * sgn, u, v
                    q = np.zeros(3)
                    q[a] = sgn
                    o.append(p)
                    d.append(q)
    for u in edge:   # inside, at the cube's first and last cells
        o.append(np.array([u, -u, 0.3]))
        d.append(np.array([0.3, -0.2, 0.9]))
    return make_rays(np.array(o, np.float32), np.array(d, np.float32))


def query_cases():
    rng = np.random.default_rng(113)
    pool = np.concatenate([special_rays(), mixed_batch(), axis_aligned_batch(), random_batch()])
    cases = []
    for flags in (0, pm.QUERY_RAW):
        for n in QUERY_N:
            cases.append((f"keys random n={n} flags={flags}", pm.case_keys(random_batch(n, seed=n), flags)))
            cases.append((f"keys pool n={n} flags={flags}", pm.case_keys(pool[rng.permutation(len(pool))[:n]], flags)))
        for name, rays in (("mixed", mixed_batch()), ("axis", axis_aligned_batch()), ("special", special_rays())):
            cases.append((f"keys {name} flags={flags}", pm.case_keys(rays, flags)))
    return cases


def all_cases():
    return tile_cases() + repeat_cases() + strip_cases() + refusal_cases() + query_cases()
