"""The models of the placement-only kernels (tests/placement_model.py) pinned by hand, on a CPU.
tests/test_gpu_placement.py compares the kernels with these models, so the models are checked first:
every expected value below stands beside the arithmetic that gives it.  Also here: the checks reject
each kind of wrong buffer the kernels could produce, the generated cases reach what they are meant
to reach, and tests/placement_driver.cpp compiles and links against the built library."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from raytracingtest_amd.query import make_rays
from tests import placement_cases as pc
from tests import placement_model as pm
from tests.conftest import ROOT

LIB_DIR = os.path.join(ROOT, "raytracingtest_amd")
G = pm.GUARD_WORDS


def _guarded(words):
    return np.concatenate([np.asarray(words, np.uint32), np.full(G, pm.GUARD, np.uint32)])


def build_driver(tmp_dir):
    """tests/placement_driver.cpp with the library's own compiler (or g++): host code only, ~2 s."""
    if not os.path.exists(os.path.join(LIB_DIR, "libsvo_rt.so")):
        pytest.skip("libsvo_rt.so not built (run __graft_entry__.build())")
    from raytracingtest_amd.build import HIPCC
    if os.path.exists(HIPCC):
        cc = [HIPCC]
    elif shutil.which("g++") and os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        cc = [shutil.which("g++"), "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
    else:
        pytest.skip("no C++ compiler with the HIP headers")
    exe = os.path.join(str(tmp_dir), "placement_driver")
    r = subprocess.run(cc + ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(LIB_DIR, "csrc"),
                             os.path.join(ROOT, "tests", "placement_driver.cpp"), "-L", LIB_DIR, "-lsvo_rt",
                             "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib",
                             "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_driver_compiles_and_links(tmp_path):
    assert os.path.exists(build_driver(tmp_path))


# ------------------------------------------------------------------ tile order
def test_tile_order_16_tiles():
    """mx = 80: class 0 is k >= 40 (2k >= 80), class 1 k >= 20, class 2 k >= 10, class 3 the rest.
    Tile 8 = 0x8005 and tile 9 = 0x8029: bit 15 is dropped, the costs are 5 and 41."""
    cost = [80, 40, 39, 20, 19, 10, 9, 0, 0x8000 | 5, 0x8000 | 41, 79, 21, 11, 1, 30, 15]
    m = pm.tile_order_model(np.array(cost, np.uint16), 16)
    assert [t.tolist() for t in m["tiles"]] == [[0, 1, 9, 10], [2, 3, 11, 14], [4, 5, 12, 15], [6, 7, 8, 13]]
    assert m["ends"].tolist() == [4, 8, 12, 16]
    # 80 + 40 + 39 + 20 + 19 + 10 + 9 + 0 + 5 + 41 + 79 + 21 + 11 + 1 + 30 + 15 = 420
    assert m["stats"].tolist() == [80, 420] + [0] * 14


def test_tile_order_odd_max():
    """mx = 81: 2k >= 81 from 41 (40: 80 < 81), 4k >= 81 from 21 (20: 80), 8k >= 81 from 11 (10: 80)."""
    m = pm.tile_order_model(np.array([81, 41, 40, 21, 20, 11, 10], np.uint16), 7)
    assert m["cls"].tolist() == [0, 0, 1, 1, 2, 2, 3]
    assert m["ends"].tolist() == [2, 4, 6, 7] and m["stats"][:2].tolist() == [81, 224]


def test_tile_order_all_zero_is_class_0():
    m = pm.tile_order_model(np.zeros(5, np.uint16), 5)   # mx = 0: 2 * 0 >= 0
    assert m["ends"].tolist() == [5, 5, 5, 5] and m["stats"][:2].tolist() == [0, 0]


def test_tile_order_check_rejects_wrong_buffers():
    cost = np.array([80, 40, 39, 20, 19, 10, 9, 0, 5, 41, 79, 21, 11, 1, 30, 15], np.uint16)
    m = pm.tile_order_model(cost, 16)
    good = _guarded([10, 9, 1, 0, 14, 11, 3, 2, 4, 5, 12, 15, 13, 8, 7, 6, 4, 8, 12, 16])   # free order inside a class
    stats = _guarded(m["stats"])
    assert pm.check_tile_order(good, stats, m) == []

    def broken(i, v, buf=good):
        b = buf.copy()
        b[i] = v
        return b
    assert pm.check_tile_order(broken(3, 1), stats, m)            # tile 0 dropped, tile 1 twice
    assert pm.check_tile_order(broken(3, 2), stats, m)            # a class 1 tile inside class 0
    assert pm.check_tile_order(broken(16, 5), stats, m)           # class end off by one
    assert pm.check_tile_order(broken(20, 0), stats, m)           # first guard word
    assert pm.check_tile_order(good, broken(1, 421, stats), m)    # wrong sum
    assert pm.check_tile_order(good, broken(2, 1, stats), m)      # stats[2..15] must be zero
    assert pm.check_tile_order(good, broken(16 + G - 1, 0, stats), m)
    heavy_last = _guarded([6, 7, 8, 13, 2, 3, 11, 14, 4, 5, 12, 15, 0, 1, 9, 10, 4, 8, 12, 16])
    assert pm.check_tile_order(heavy_last, stats, m)              # the heavy tiles at the back of the list


# ------------------------------------------------------------------ strip order
def _blocks(m, x):
    return [(b["start"], b["end"], b["tiles"].tolist()) for b in m["xcds"][x]["blocks"]]


def test_strip_order_8x2_thresholds():
    """XCD x owns the column x: tile x (row 0, cost 64 = the XCD's max) and tile 8 + x (row 1).  Against
    mx = 64 the thresholds are 7/8: 56, 3/4: 48, 1/2: 32, 1/4: 16 (and 1/8: 8, in the 8x3 case below)."""
    row1 = [56,   # 8 * 56 = 448 >= 7 * 64 = 448: class 0
            55,   # 440 < 448; 4 * 55 = 220 >= 192: class 1
            48,   # 4 * 48 = 192 >= 192: class 1
            47,   # 188 < 192; 2 * 47 = 94 >= 64: class 2
            32,   # 2 * 32 = 64 >= 64: class 2
            31,   # 62 < 64; 4 * 31 = 124 >= 64: class 3
            16,   # 4 * 16 = 64 >= 64: class 3
            15]   # 60 < 64; 8 * 15 = 120 >= 64: class 4
    m = pm.strip_order_model(np.array([64] * 8 + row1, np.uint16), 16, 8)
    assert (m["L"], m["G"]) == (2, 16)
    want_cls = [0, 1, 1, 2, 2, 3, 3, 4]
    for x in range(8):
        blocks = _blocks(m, x)
        tiles = [[] for _ in range(6)]
        tiles[0].append(x)
        tiles[want_cls[x]].append(8 + x)
        assert [b[2] for b in blocks] == tiles, x
        ends = np.cumsum([len(t) for t in tiles]).tolist()
        assert [b[1] for b in blocks] == ends, x
        assert m["stats"][2 * x] == 64 and m["stats"][2 * x + 1] == 64 + row1[x]
    # the prio class ends (classes 2 .. 5) as the render kernel reads them
    o = pm.strip_order_layout(m)
    assert o[16:20].tolist() == [0, 0, 0, 0]
    assert o[20:52].reshape(8, 4).tolist() == [[2, 2, 2, 2]] * 5 + [[1, 2, 2, 2]] * 2 + [[1, 1, 2, 2]]
    assert pm.check_strip_order(_guarded(o), _guarded(m["stats"]), m) == []


def test_strip_order_8x3_every_threshold_and_its_predecessor():
    """Three tiles per XCD: x (row 0), 8 + x (row 1), 16 + x (row 2).  XCDs 0 .. 4: the max 63 (odd), a tile on
    one threshold and the tile just below it: 8k >= 441 from 56, 4k >= 189 from 48, 2k >= 63 from 32,
    4k >= 63 from 16, 8k >= 63 from 8.  XCD 5: two zero tiles (class 5); XCD 6: all zero (mx = 0: class 0);
    XCD 7: mx = 1, so 1 is class 0 and 0 (8 * 0 < 1) class 5."""
    rows = [[63, 63, 63, 63, 63, 63, 0, 1],
            [56, 48, 32, 16, 8, 0, 0, 1],
            [55, 47, 31, 15, 7, 0, 0, 0]]
    m = pm.strip_order_model(np.array(rows, np.uint16).reshape(-1), 24, 8)
    e = []
    want = {0: [[0, 8], [16], e, e, e, e],        # 55: 440 < 441, 220 >= 189
            1: [[1], [9], [17], e, e, e],         # 47: 188 < 189, 94 >= 63
            2: [[2], e, [10], [18], e, e],        # 31: 62 < 63, 124 >= 63
            3: [[3], e, e, [11], [19], e],        # 15: 60 < 63, 120 >= 63
            4: [[4], e, e, e, [12], [20]],        # 7: 56 < 63
            5: [[5], e, e, e, e, [13, 21]],
            6: [[6, 14, 22], e, e, e, e, e],
            7: [[7, 15], e, e, e, e, [23]]}
    for x in range(8):
        assert [b[2] for b in _blocks(m, x)] == want[x], x
    # stats: max and sum per XCD
    assert m["stats"].tolist() == [63, 174, 63, 158, 63, 126, 63, 94, 63, 78, 63, 63, 0, 0, 1, 2]
    o = pm.strip_order_layout(m)
    assert o[28:60].reshape(8, 4).tolist() == [[3, 3, 3, 3], [3, 3, 3, 3], [2, 3, 3, 3], [1, 2, 3, 3], [1, 1, 2, 3],
                                               [1, 1, 1, 3], [3, 3, 3, 3], [2, 2, 2, 3]]


def test_strip_order_spread_classes_by_the_neighbourhood():
    """16 x 2 tiles, one heavy tile (100) at row 0, column 7; everything else 1.  Without spread XCD 7 has
    tile 7 in class 0 and its other three tiles (1: 8 < 100) in class 5.  With spread the tiles of the
    columns 6 .. 8 take cost 100: XCD 6 (columns 6, 14; own max 1) classes against 1 -- all four class 0
    anyway; XCD 7 gets tiles 7 and 23 in class 0; XCD 0 (columns 0, 8; own max 1) stays all class 0.  The
    stats stay those of the tiles themselves."""
    cost = np.ones(32, np.uint16)
    cost[7] = 100
    m0 = pm.strip_order_model(cost, 32, 16)
    assert [b[2] for b in _blocks(m0, 7)] == [[7], [], [], [], [], [15, 23, 31]]
    m1 = pm.strip_order_model(cost, 32, 16, spread=1)
    assert [b[2] for b in _blocks(m1, 7)] == [[7, 23], [], [], [], [], [15, 31]]
    assert [b[2] for b in _blocks(m1, 6)][0] == [6, 14, 22, 30] and [b[2] for b in _blocks(m1, 0)][0] == [0, 8, 16, 24]
    assert m1["stats"].tolist() == m0["stats"].tolist() == [1, 4] * 7 + [100, 103]


def test_strip_order_seg_cap_smaller_than_the_top_class():
    """8 x 4 tiles (4 per XCD), kpack 0x84: class 0 in quarters (K = 4), class 1 in eighths (K = 8), seg_cap 2.
    kmax = 8, so L = 4 + 7 * 2 = 18 and G = 144.
    XCD 0: 100, 100, 100, 80.  8k >= 700 from 88: tiles 0, 8, 16 are class 0, 80 (320 >= 300) class 1.
      Class 0 gets min(3, 2) = 2 segmented tiles -> block [0, 3 + 3 * 2 = 9); nothing is left for class 1:
      block [9, 10).
    XCD 1: 100, 80, 80, 10.  Class 0 = {1}: 1 segmented, block [0, 4), 1 left; class 1 = {9, 17}: min(2, 1) = 1
      segmented in 8 parts, block [4, 4 + 2 + 7 = 13); 10 (80 < 100) is class 5: [13, 14).
    XCDs 2 .. 7: all zero, mx = 0: four class 0 tiles, 2 segmented: [0, 4 + 6 = 10)."""
    c = np.zeros((4, 8), np.uint16)
    c[:, 0] = [100, 100, 100, 80]
    c[:, 1] = [100, 80, 80, 10]
    m = pm.strip_order_model(c.reshape(-1), 32, 8, seg_cap=2, kpack=0x84)
    assert (m["L"], m["G"], m["kmax"]) == (18, 144, 8)
    b = m["xcds"][0]["blocks"]
    assert [(v["start"], v["end"], v["segs"]) for v in b] == [(0, 9, 2), (9, 10, 0)] + [(10, 10, 0)] * 4
    b = m["xcds"][1]["blocks"]
    assert [(v["start"], v["end"], v["segs"]) for v in b] == [(0, 4, 1), (4, 13, 1), (13, 13, 0), (13, 13, 0),
                                                             (13, 13, 0), (13, 14, 0)]
    assert [(v["start"], v["end"], v["segs"]) for v in m["xcds"][5]["blocks"]] == [(0, 10, 2)] + [(10, 10, 0)] * 5
    # one layout the kernel may write, entry by entry, for XCD 1 (list entry j is order[8 j + 1])
    o = pm.strip_order_layout(m)
    E = pm.SEG_EMPTY
    assert o[1:144:8].tolist() == ([1 | q << 28 for q in (1, 2, 3, 4)] + [9 | q << 28 for q in range(5, 13)] +
                                   [17, 25] + [E] * 4)
    assert o[144:148].tolist() == [0] * 4 and o[148 + 4:148 + 8].tolist() == [13, 13, 13, 14]
    stats = _guarded(m["stats"])
    assert pm.check_strip_order(_guarded(o), stats, m) == []
    # the one freedom: WHICH tiles of a class are the segmented ones
    assert pm.check_strip_order(_guarded(pm.strip_order_layout(m, pick_last=True)), stats, m) == []

    def broken(edit):
        bad = o.copy()
        edit(bad.reshape(-1))
        return pm.check_strip_order(_guarded(bad), stats, m)

    def put(i, v):
        return lambda a: a.__setitem__(i, v)
    assert broken(put(8 * 1 + 1, 1 | 4 << 28))         # part codes not ascending
    assert broken(put(8 * 3 + 1, 9 | 4 << 28))         # a group over two tiles
    assert broken(put(8 * 4 + 1, 17 | 5 << 28))        # tile 9's first part lost, tile 17 twice
    assert broken(put(8 * 12 + 1, 9))                  # a tile both segmented and plain
    assert broken(put(8 * 12 + 1, E))                  # a tile dropped
    assert broken(put(8 * 14 + 1, 25))                 # padding is not SEG_EMPTY
    assert broken(put(148 + 4, 12))                    # class end off by one
    assert broken(put(145, 7))                         # global bounds
    assert broken(lambda a: a.__setitem__(slice(0, 8 * 4, 8), [0, 8, 0 | 1 << 28, 0 | 2 << 28]))   # 3 parts of 4
    # three segmented tiles where the cap allows two
    three = o.copy()
    three[0:144:8] = ([0 | q << 28 for q in (1, 2, 3, 4)] + [8 | q << 28 for q in (1, 2, 3, 4)] +
                      [16 | q << 28 for q in (1, 2, 3, 4)] + [24] + [E] * 5)
    assert pm.check_strip_order(_guarded(three), stats, m)
    bad_stats = stats.copy()
    bad_stats[3] += 1
    assert pm.check_strip_order(_guarded(o), bad_stats, m)
    bad_guard = _guarded(o)
    bad_guard[-1] = 0
    assert pm.check_strip_order(bad_guard, stats, m)


def test_strip_order_flagged_tiles_take_part_costs():
    """A word with SEG_COST_FLAG: the cost is the max of the first 4 part costs, of all 8 when word & 15 == 8;
    0xFFFF in the unused slots must not be read.  With part_cost null the word's low 15 bits count."""
    cost = np.array([0x8004, 0x8008, 50, 0x8004], np.uint16)
    part = np.full((4, 8), 0xFFFF, np.uint16)
    part[0, :4] = [7, 300, 2, 9]
    part[1] = [1, 2, 3, 4, 5, 600, 7, 8]
    part[3, :4] = [0, 0, 0, 0]
    assert pm.tile_costs(cost, 4, part.reshape(-1)).tolist() == [300, 600, 50, 0]
    assert pm.tile_costs(cost, 4, None).tolist() == [4, 8, 50, 4]


def test_strip_refusals():
    assert pm.strip_refusal(64, 8, 1, 0x3) and pm.strip_refusal(64, 8, 0, 0xF00000)
    assert not pm.strip_refusal(64, 8, 1, 0x848400)
    assert pm.strip_refusal(24, 16, 1, 0x4) and not pm.strip_refusal(24, 16, 0, 0x4)
    # grid = n + 8 (K - 1) seg_cap: 64 + 24 * 11184808 = 268435456 = 2^28, refused; 64 + 24 * 11184807 is 24 less
    assert pm.strip_refusal(64, 8, 11184808, 0x4) and not pm.strip_refusal(64, 8, 11184807, 0x4)
    assert [c["refused"] for _, c in pc.refusal_cases()] == [True] * 4
    assert pm.seg_kmax_of(0) == 1 and pm.seg_kmax_of(0x448) == 8 and pm.order_strips_entries(32400, 96, 8) == 37812
    assert pm.order_cost_capacity(1) == 32768 and pm.order_cost_capacity(32769) == 65536


# ------------------------------------------------------------------ query keys
def test_query_keys_by_hand():
    """World [-16, 16]^3 is the cube [1, 2]^3: s = w / 32 + 1.5.  The clamp turns a zero direction component
    into 2^-23 (coef = -2^23), which never bounds t here.
    A  origin (-40, 8, -4), direction +x: s = (0.25, 1.75, 1.375); the -x face is at t = (1 - 0.25) / 1 =
       0.75 (t_max = 1.75).  Entry x = 0.25 + 0.75 = 1 -> cell 0; y = 1.75 + 0.75 * 2^-23 rounds up to
       1.75 + 2^-23 -> (0.75 + 2^-23) * 512 -> cell 384; z likewise 0.375 * 512 -> cell 192.  All three
       components positive: octant mask 7 ^ 1 ^ 2 ^ 4 = 0.
       384 = bits 8, 7 -> key bits 3 * 8 + 1 = 25 and 22; 192 = bits 7, 6 -> key bits 23 and 20: 0x2D00000.
    B  origin (4, -8, 12) inside, direction (-1, -1, -1): s = (1.625, 1.25, 1.875), t_min = max(-0.375, -0.75,
       -0.125, 0) = 0, t_max = 0.25: the entry point is the origin, cells (320, 128, 448); octant mask 7.
       320 = bits 8, 6 -> 24, 18; 128 = bit 7 -> 22; 448 = bits 8, 7, 6 -> 26, 23, 20: 0x5D40000 | 7 << 27.
    C  origin (-40, 40, 0), direction +x: s_y = 2.75; the y slab ends at t = -2^23 + 2^23 * (3 - 2.75) < 0
       before x enters at 0.75: t_min > t_max, no key."""
    rays = make_rays([(-40.0, 8.0, -4.0), (4.0, -8.0, 12.0), (-40.0, 40.0, 0.0)],
                     [(1.0, 0.0, 0.0), (-1.0, -1.0, -1.0), (1.0, 0.0, 0.0)])
    assert pm.query_keys_model(rays).tolist() == [0x2D00000, 0x5D40000 | 7 << 27, (1 << 30) - 1]
    # raw: the zero components of A and C stay zero -- coef = -inf, bias = -inf, every y and z bound is
    # -inf + inf = NaN and drops out of the min / max, so x alone decides: t_min = 0.75 <= t_max = 1.75.
    # A enters at (1, 1.75, 1.375) exactly, the same cells; C now "enters" at y = 2.75 -> 1.75 * 512 = 896,
    # clamped to cell 511 (bits 3 i + 1: 0o222222222), z = 1.5 -> cell 256 (bit 26).  Octant mask 7 ^ 1 = 6
    # (a zero component is not positive).
    assert pm.query_keys_model(rays, pm.QUERY_RAW).tolist() == [0x2D00000 | 6 << 27, 0x5D40000 | 7 << 27,
                                                                0o222222222 | 1 << 26 | 6 << 27]


def test_morton27():
    assert pm.morton27(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [256, 0, 0], [511, 511, 511], [0, 0, 511]])).tolist() \
        == [1, 2, 4, 1 << 24, (1 << 27) - 1, 0o444444444]


def test_query_keys_invalid_rays_get_no_key():
    rays = make_rays(np.zeros((5, 3)), [(0, 0, 0), (np.nan, 0, 1), (np.inf, 0, 1), (0, 0, 1), (0, 0, 1)])
    rays["origin"][3, 1] = np.inf
    rays["t_max"][4] = np.nan
    assert pm.query_keys_model(rays).tolist() == [pm.KEY_NONE] * 5


def test_query_check_rejects_wrong_buffers():
    keys = np.array([5, 3, 5, 1], np.uint32)
    idx = np.arange(4, dtype=np.uint32)
    g = _guarded
    assert pm.check_query_keys(g(keys), g(idx), g([1, 3, 5, 5]), g([3, 1, 2, 0]), keys) == []   # stability not required
    assert pm.check_query_keys(g(keys), g(idx), g([1, 3, 5, 5]), g([3, 1, 0, 2]), keys) == []
    assert pm.check_query_keys(g([5, 3, 4, 1]), g(idx), g([1, 3, 4, 5]), g([3, 1, 2, 0]), keys)     # wrong key
    assert pm.check_query_keys(g(keys), g(idx), g([3, 1, 5, 5]), g([1, 3, 2, 0]), keys)             # not sorted
    assert pm.check_query_keys(g(keys), g(idx), g([1, 3, 5, 5]), g([3, 1, 2, 2]), keys)             # no permutation
    assert pm.check_query_keys(g(keys), g(idx), g([1, 3, 5, 5]), g([1, 3, 2, 0]), keys)             # pairs torn apart
    assert pm.check_query_keys(g(keys), g([0, 1, 2, 2]), g([1, 3, 5, 5]), g([3, 1, 2, 0]), keys)
    assert pm.check_query_keys(g(keys), g(idx), g([1, 3, 5, 5]), np.append(g([3, 1, 2, 0])[:-1], 0), keys)   # guard


# ------------------------------------------------------------------ the generated cases
def test_generated_cases_reach_what_they_are_meant_to():
    """Heavy-tailed costs populate every class; the seg_cap values lie above, on and below the sizes of the
    classes they segment; the ladders put a tile on every threshold and one just below; the key batches hold
    entry cells 0 and 511 on every axis, inside origins, invalid rays and rays that miss."""
    for name, c in pc.tile_cases():
        m = pm.tile_order_model(c["cost"], c["n"])
        if c["n"] >= 2047 and ("heavy" in name or "ladder" in name):
            assert np.all(np.diff(np.concatenate([[0], m["ends"]])) > 0), name
        if "bit15" in name and c["n"] >= 31:
            assert np.any(c["cost"] & 0x8000) and m["stats"][0] < 0x8000
    rel = set()
    flagged_k = set()
    for name, c in pc.strip_cases():
        m = pm.strip_order_model(c["cost"], c["n"], c["tiles_x"], c["seg_cap"], c["kpack"], c["spread"], c["part_cost"])
        ln = c["n"] // 8
        for xc in m["xcds"]:
            if ("heavy" in name and ln >= 1000) or ("ladder" in name and ln >= 11 and not c["spread"]):
                assert all(len(b["tiles"]) > 0 for b in xc["blocks"]), name
            left = c["seg_cap"]
            for b in xc["blocks"]:
                if b["K"] > 1 and len(b["tiles"]):
                    rel.add("above" if left > len(b["tiles"]) else "equal" if left == len(b["tiles"]) else
                            "none left" if left == 0 else "below")
                    left -= b["segs"]
        if c["part_cost"] is not None:
            flagged_k |= set((c["cost"][(c["cost"] & 0x8000) != 0] & 15).tolist())
        if "ladder" in name and c["n"] // 8 >= 11 and not c["spread"]:
            mx = int(name.split("ladder")[1])
            for x in range(8):
                own = set(c["cost"].reshape(-1, c["tiles_x"])[:, x::8].reshape(-1).tolist())
                assert set(pc.ladder(mx).tolist()) <= own, name
    assert rel == {"above", "equal", "below", "none left"}, rel
    assert flagged_k == {4, 8}
    cells = set()
    kinds = set()
    for name, c in pc.query_cases():
        keys = pm.query_keys_model(c["rays"], c["flags"])
        kinds |= {"none"} if np.any(keys == pm.KEY_NONE) else set()
        kinds |= {"entered"} if np.any(keys != pm.KEY_NONE) else set()
        k = keys[keys != pm.KEY_NONE]
        for a in range(3):
            g = sum(((k >> np.uint32(3 * i + a)) & 1) << i for i in range(9))
            cells |= {(a, int(v)) for v in np.unique(g) if v in (0, 511)}
    assert cells == {(a, v) for a in range(3) for v in (0, 511)} and kinds == {"none", "entered"}


def test_case_file_round_trip(tmp_path):
    """write_cases' layout is what placement_driver.cpp reads: kind, 8 parameters, two blob lengths, the blobs."""
    cases = [c for _, c in pc.refusal_cases()[:1]] + [pm.case_tiles(np.arange(5, dtype=np.uint16), 5)]
    path = tmp_path / "cases.bin"
    pm.write_cases(path, cases)
    w = np.fromfile(path, "<u4")
    assert w[:2].tolist() == [pm.MAGIC, 2]
    assert w[2:13].tolist() == [1, 64, 8, 1, 0x3, 0, 0, pm.HIP_INVALID_VALUE, 1, 32, 0]
    assert w[13 + 32:13 + 32 + 11].tolist() == [0, 5, 1, 0, 0, 0, 0, 0, 0, 3, 0]
    assert w[13 + 32 + 11:].view(np.uint16).tolist() == [0, 1, 2, 3, 4, 0]
