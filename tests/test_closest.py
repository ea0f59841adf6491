"""Closest-voxel queries without a GPU: the rule's header (csrc/svo_closest.h, built by plain g++ into
tests/closest_driver.cpp) against its Python statement (closest.closest_model) byte for byte, the model against a
brute force over all result voxels (closest.closest_bruteforce) and against float64 geometry, conditions on the
batch so that no test passes on degenerate inputs, and the C API's argument errors from the loaded library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from raytracingtest_amd import _lib
from raytracingtest_amd import closest as cl
from raytracingtest_amd import overlap as ov
from tests import closest_util as cu
from tests import geometry_model as gm
from tests import overlap_util as ou
from tests.conftest import ROOT
from tests.test_overlap import guard_svo

NAMES = ("svo_closest_voxels", "svo_closest_voxels_host")
CASES = [(name, coarse, unbounded) for name in cu.POOLS for coarse in cu.COARSE[name] for unbounded in (False, True)]


@pytest.fixture(scope="module")
def native():
    from raytracingtest_amd import build
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("closest") / "closest_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "closest_driver.cpp"), "-o", str(exe)], check=True)

    def run(svo, queries, root=0, flags=0, max_visits=0, coarse_level=0, exe=exe):
        d = tmp_path_factory.mktemp("run")
        svo.to_v2().astype("<u8").tofile(d / "nodes.bin")
        np.ascontiguousarray(queries, cl.SHAPE_DTYPE).tofile(d / "queries.bin")
        subprocess.run([str(exe), str(d / "nodes.bin"), str(d / "queries.bin"), str(d / "nearest.bin"), str(d / "contacts.bin"),
                        str(root), str(flags), str(max_visits), str(coarse_level)], check=True)
        return np.fromfile(d / "nearest.bin", cl.CLOSEST_DTYPE), np.fromfile(d / "contacts.bin", cl.CONTACT_DTYPE)
    return run


# ------------------------------------------------------------------------------------ the surface
def test_symbols_layouts_and_abi(native, tmp_path):
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(native, name)
    assert native.svo_abi_version() == _lib.ABI_VERSION == 10
    src = tmp_path / "t.c"
    src.write_text('#include "svo_rt.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(svo_closest) == 32 && offsetof(svo_closest, d2) == 12 && offsetof(svo_closest, parent) == 16 '
                   '&& offsetof(svo_closest, meta) == 20 && offsetof(svo_closest, visits) == 24 && offsetof(svo_closest, flags) == 28, "closest");\n'
                   '_Static_assert(sizeof(svo_closest_params) == 20 && offsetof(svo_closest_params, root) == 8 '
                   '&& offsetof(svo_closest_params, max_visits) == 12 && offsetof(svo_closest_params, coarse_level) == 16, "params");\n'
                   '_Static_assert(sizeof(svo_closest_out) == 3 * sizeof(void *) && offsetof(svo_closest_out, hitmask) == 2 * sizeof(void *), "out");\n'
                   '_Static_assert(SVO_CLOSEST_UNBOUNDED == 1, "enums");\n'
                   'int main(void){return 0;}\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "t")], check=True)
    assert ctypes.sizeof(_lib.SvoClosestParams) == 20 and ctypes.sizeof(_lib.SvoClosestOut) == 3 * ctypes.sizeof(ctypes.c_void_p)
    f = cl.CLOSEST_DTYPE.fields
    assert [f[k][1] for k in ("point", "d2", "parent", "meta", "visits", "flags")] == [0, 12, 16, 20, 24, 28]


def test_csharp_shim_declares_the_calls():
    text = open(os.path.join(ROOT, "unity", "RaytracingMasterNative.cs")).read()
    for name in NAMES:
        assert re.search(rf"\[DllImport\(Lib\)\] public static extern int {name}\(", text), name
    assert "public int ClosestVoxels(" in text
    # no C# toolchain here: each struct has the header's fields, in order, as 4-byte words
    for struct, words in (("SvoClosest", 8), ("SvoClosestParams", 5)):
        body = re.search(rf"public struct {struct}\s*\{{(.*?)\n    \}}", text, re.S)
        assert body, struct
        got = 0
        for kind, names in re.findall(r"public (float|uint|ulong) ([\w, ]+);", body.group(1)):
            got += (2 if kind == "ulong" else 1) * len(names.split(","))
        assert got == words, (struct, got)


def test_argument_errors_without_a_gpu(native):
    """Every SVO_ERR_ARG of the two calls, on a zeroed fake context (capacity 0, no pool): no call reaches a
    device.  The root test stands last among the parameter tests, so the fake context's capacity of 0 shows it."""
    fake = ctypes.create_string_buffer(1 << 20)
    ctx = ctypes.addressof(fake)
    raw = np.zeros(4096 + 64, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data % 64)
    queries, nearest, contacts = base, base + 1024, base + 2048
    P = _lib.closest_params
    out = lambda s=nearest, c=None, m=None: ctypes.byref(_lib.SvoClosestOut(s, c, m))   # noqa: E731

    def dev(ctx_=ctx, queries_=queries, n=4, prm=P(), out_=None):
        return native.svo_closest_voxels(ctx_, queries_, n, ctypes.byref(prm) if prm is not None else None,
                                         out() if out_ is None else out_, None)

    def host(ctx_=ctx, queries_=queries, n=4, prm=P(), nearest_=nearest, contacts_=None):
        return native.svo_closest_voxels_host(ctx_, queries_, n, ctypes.byref(prm) if prm is not None else None, nearest_,
                                              contacts_)

    def err():
        return native.svo_last_error().decode()

    assert dev(ctx_=None) == -1 and "null context" in err()
    assert dev(queries_=None) == -1 and "null query list" in err()
    assert native.svo_closest_voxels(ctx, queries, 4, ctypes.byref(P()), None, None) == -1 and "null svo_closest_out" in err()
    assert dev(out_=out(None, None, None)) == -1 and "every closest output is null" in err()
    assert host(ctx_=None) == -1 and host(queries_=None) == -1
    assert host(nearest_=None) == -1 and "every closest output is null" in err()
    for call in (dev, host):
        assert call(prm=P(unbounded=True)) == -1 and "root" in err()     # a good flag passes the flag test
        bad = P()
        bad.flags = 2
        assert call(prm=bad) == -1 and "unknown closest flag bits" in err()
        assert call(prm=P(max_visits=(1 << 24) + 1)) == -1 and "max_visits" in err()
        assert call(prm=P(coarse_level=23)) == -1 and "coarse_level" in err()
        small = P()
        small.size = 4
        assert call(prm=small) == -1 and "size" in err()
        big = P()
        big.size = 24
        assert call(prm=big) == -1 and "newer ABI" in err()
        # root >= capacity: the fake context's capacity is 0, so every root is outside
        assert call(prm=P(root=0)) == -1 and "root outside the node-pool capacity" in err()
        assert call(prm=None) == -1 and "root outside the node-pool capacity" in err()   # NULL params: the defaults
    assert host(contacts_=contacts) == -1 and "root outside" in err()                    # contacts need no K
    assert bytes(fake) == bytes(1 << 20) and not raw.any()


def test_count_limits_without_a_gpu(native):
    """n above 2^31 - 1: the count test stands before the root test, so the zeroed context shows it; the largest
    count that passes it ends at the root test (capacity 0), not at a device."""
    fake = ctypes.create_string_buffer(1 << 20)
    ctx = ctypes.addressof(fake)
    raw = np.zeros(256, np.uint8)
    queries = raw.ctypes.data + (-raw.ctypes.data % 16)
    P = _lib.closest_params
    host = lambda n: native.svo_closest_voxels_host(ctx, queries, n, ctypes.byref(P()), queries + 64, None)   # noqa: E731
    assert host(1 << 31) == -1 and b"2^31 - 1 queries" in native.svo_last_error()
    assert host((1 << 31) - 1) == -1 and b"root outside" in native.svo_last_error()
    out = _lib.SvoClosestOut(queries + 64, None, None)
    assert native.svo_closest_voxels(ctx, queries, 1 << 31, ctypes.byref(P()), ctypes.byref(out), None) == -1
    assert b"2^31 - 1 queries" in native.svo_last_error()
    assert bytes(fake) == bytes(1 << 20) and not raw.any()


# ------------------------------------------------------------------------------------ the batch
def tie_counts(rows, queries):
    """Per query (how many result voxels have the smallest f32 d2, that d2), over all rows, no radius."""
    lo, hi = cl.voxel_boxes(rows)
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    out = []
    with np.errstate(all="ignore"):
        for q in queries:
            d2 = cu._f32_d2(lo32, hi32, q["p"])
            out.append((int(np.count_nonzero(d2 == d2.min())), float(d2.min())))
    return out


@pytest.mark.parametrize("name", cu.POOLS)
def test_batch_conditions(name):
    """The batch is what its docstring says: zero distances shared by several voxels, ties at d2 > 0 that the
    Morton order decides, radii on either side of the distance, points outside, invalid queries."""
    queries, parts = cu.batch(name)
    rows = cu.voxels(name)
    near, con, mask = cu.model(name)
    free, _, _ = cu.model(name, unbounded=True)
    found = (near["flags"] & 1) != 0
    assert (near["d2"][parts["centre"]] == 0).all() and found[parts["centre"]].all()
    ties = tie_counts(rows, queries[parts["face"]])
    assert all(d == 0 for _, d in ties) and sum(k >= 2 for k, _ in ties) >= 8, "points on faces shared by several voxels"
    ties = tie_counts(rows, queries[parts["gap"]])
    assert len(ties) == 30 and all(k >= 2 and d > 0 for k, d in ties), "equal non-zero d2: the tie-break decides"
    outside = near[parts["outside"]]
    assert (outside["flags"][:4] == 1).all() and (outside["d2"][:4] > 0).all()
    assert outside["flags"][4] == 0 and outside["flags"][5] == 0, "r r finite against d2 = +inf; a radius too small"
    assert free["flags"][parts["outside"]][4] == 1 and np.isinf(free["d2"][parts["outside"]][4])
    zero = near[parts["zero"]]
    assert (zero["flags"][:4] == 1).all() and (zero["d2"][:4] == 0).all() and (zero["flags"][4:] == 0).all()
    rad = near[parts["radius"]]
    assert (rad["flags"][0::2] == 1).all() and (rad["flags"][1::2] == 0).all(), "r r >= d2 finds, the next smaller r does not"
    assert (free[parts["radius"]]["flags"] == 1).all()
    assert (free[parts["radius"]][0::2]["d2"] == rad["d2"][0::2]).all()
    assert (near["flags"][parts["invalid"]] == 0x10).all() and (near["visits"][parts["invalid"]] == 0).all()
    valid = cl.queries_valid(queries)
    assert valid.sum() == cu.N - 6 and (free["flags"][valid] == 1).all() and (free["flags"][~valid] == 0x10).all()
    assert 10 <= np.count_nonzero(found[parts["fill"]]) <= len(queries[parts["fill"]]) - 5
    # not found: the record and the contact of nothing
    none = near[valid & ~found]
    assert (none["d2"] == np.inf).all() and (none["parent"] == 0xFFFFFFFF).all() and not none["point"].any() and not none["meta"].any()
    assert con[~found].tobytes() == ov.unused_contacts(int((~found).sum())).tobytes()
    assert (con["parent"][found] == near["parent"][found]).all() and (con["meta"][found] == near["meta"][found]).all()


@pytest.mark.parametrize("name,coarse,unbounded", CASES)
def test_model_equals_bruteforce(name, coarse, unbounded):
    """Branch and bound equals the brute force over all result voxels under the same f32 rule, byte for byte:
    voxel, d2, point, contact and mask.  Nothing on these pools carries the budget or the overflow flag."""
    queries, parts = cu.batch(name)
    rows = cu.voxels(name, coarse)
    near, con, mask = cu.model(name, unbounded, coarse)
    assert not (near["flags"] & (cl.FLAG_BUDGET | cl.FLAG_OVERFLOW)).any()
    want, want_con = cl.closest_bruteforce(rows, queries, flags=cl.CLOSEST_UNBOUNDED if unbounded else 0)
    got = near.copy()
    got["visits"] = 0
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:8]
    assert con.tobytes() == want_con.tobytes()
    found = (near["flags"] & 1) != 0
    want_mask = np.zeros_like(mask)
    for s in np.flatnonzero(found):
        want_mask[s // 64] |= np.uint64(1 << (s % 64))
    assert (mask == want_mask).all()
    valid = cl.queries_valid(queries)
    assert (near["visits"][valid] >= 1).all() and (near["visits"][~valid] == 0).all()
    if coarse == 0:
        # the answer is a leaf of the pool, named as a ray hit names it; a point in the middle of a leaf at
        # level L walks one path of L descriptors when nothing ties with it
        leaves = gm.pool(name)[1]
        keys = {(int(r[0]), int(r[1])): (int(r[2]), int(k)) for r, k in zip(leaves, gm.voxel_keys(leaves))}
        for s in np.flatnonzero(found):
            level, key = keys[(int(con[s]["parent"]), int(con[s]["meta"] & 0xFF))]
            assert (con[s]["meta"] >> 8) == 23 - level and int(con[s]["key"]) == key
        c = near[parts["centre"]]
        assert (c["visits"] == 23 - (c["meta"] >> 8)).all()
    else:
        assert (23 - (near["meta"][found] >> 8) <= coarse).all() and (23 - (near["meta"][found] >> 8) == coarse).sum() >= 50


def test_model_equals_bruteforce_on_the_text_pool(text_svo):
    """The golden text pool (4,977 descriptors), its own batch, bounded and unbounded, leaves and a coarse level."""
    leaves = text_svo.leaf_voxels()
    queries, parts = cu.make_batch(leaves, 4977)
    for coarse in (0, 5):
        rows = leaves if coarse == 0 else cl.result_voxels(text_svo, coarse)
        if coarse == 0:
            assert sorted(map(tuple, cl.result_voxels(text_svo))) == sorted(map(tuple, leaves))
        for flags in (0, cl.CLOSEST_UNBOUNDED):
            near, con, _ = cl.closest_model(text_svo, queries, flags=flags, coarse_level=coarse)
            want, want_con = cl.closest_bruteforce(rows, queries, flags=flags)
            assert not (near["flags"] & (cl.FLAG_BUDGET | cl.FLAG_OVERFLOW)).any()
            near["visits"] = 0
            assert near.tobytes() == want.tobytes() and con.tobytes() == want_con.tobytes(), (coarse, flags)
            assert ((near["flags"] & 1) != 0).sum() >= (100 if not flags else cu.N - 6)


@pytest.mark.parametrize("name", cu.POOLS)
def test_morton_order_is_the_overlap_walks_order(name):
    """closest.morton_before (the header's comparison) and closest.morton_code agree, and both put the contacts of
    svo_overlap_volumes' model in the order in which its walk reports them."""
    _, contacts, _ = ou.model(name)
    summary = ou.model(name)[0]
    checked = 0
    for s in np.flatnonzero(summary["count"] >= 2)[:40]:
        got = contacts[s, :min(int(summary["count"][s]), 32)]
        vox = [(23 - (int(c["meta"]) >> 8), [(int(c["key"]) >> (21 * k)) & 0x1FFFFF for k in range(3)]) for c in got]
        for a, b in zip(vox, vox[1:]):
            assert cl.morton_before(*a, *b) and not cl.morton_before(*b, *a)
            assert cl.morton_code(*a) < cl.morton_code(*b)
            checked += 1
    assert checked >= 200


@pytest.mark.parametrize("name,coarse", [(n, c) for n in cu.POOLS for c in cu.COARSE[n]])
def test_found_bit_is_overlaps_touch_bit(name, coarse):
    """The same shapes through overlap.overlap_model: something found == the sphere touches a voxel.  Both batches:
    the closest queries, and overlap's own shapes (its boxes are invalid queries here, and found nowhere)."""
    svo = gm.pool(name)[0]
    queries, _ = cu.batch(name)
    near, _, mask = cu.model(name, False, coarse)
    touch, _, touch_mask = ov.overlap_model(svo, queries, flags=ov.OVERLAP_ANY, coarse_level=coarse)
    box = queries["kind"] == 0       # the batch's one box: a shape for overlap, no query here
    assert box.sum() == 1 and (near["flags"][box] == 0x10).all() and (touch["flags"][box] == 1).all()
    assert (near["flags"] & 0x11)[~box].tobytes() == (touch["flags"] & 0x11)[~box].tobytes()
    bit = np.uint64(1 << int(np.flatnonzero(box)[0]) % 64)
    touch_mask = touch_mask.copy()
    touch_mask[int(np.flatnonzero(box)[0]) // 64] &= ~bit
    assert (mask == touch_mask).all()
    shapes, _ = ou.batch(name)
    sphere = shapes["kind"] == 1
    got, _, _ = cl.closest_model(svo, shapes, coarse_level=coarse)
    want = ou.model(name, True, coarse)[0]
    assert ((got["flags"] & 1) == (want["flags"] & 1))[sphere].all() and (got["flags"] & 1)[sphere].sum() >= 20
    assert (got["flags"][shapes["kind"] == 0] == 0x10).all()


@pytest.mark.parametrize("name,coarse", [(n, c) for n in cu.POOLS for c in cu.COARSE[n]])
def test_distance_against_float64(name, coarse):
    """d2 and the chosen voxel's true squared distance are within D2_REL_BOUND = 11 * 2^-24 (derived in
    svo_closest.h from the rule's five roundings) of the true float64 minimum over all result voxels; the closest
    point lies on the chosen voxel's box at that true distance."""
    queries, _ = cu.batch(name)
    rows = cu.voxels(name, coarse)
    near, con, _ = cu.model(name, True, coarse)
    index = {(int(r[0]), int(r[1])): j for j, r in enumerate(rows)}
    assert cl.D2_REL_BOUND == 11 * 2.0 ** -24
    checked = 0
    for s in np.flatnonzero((near["flags"] & 1) != 0):
        p = queries[s]["p"].astype(np.float64)
        if not np.all(np.abs(p) < 1e6):
            continue                                  # the far point: e e overflows, outside the bound's premise
        D = cl.true_d2(rows, p)
        Dmin = D.min()
        j = index[(int(near[s]["parent"]), int(near[s]["meta"] & 0xFF))]
        tol = cl.D2_REL_BOUND * Dmin
        assert abs(float(near[s]["d2"]) - Dmin) <= tol, (s, float(near[s]["d2"]), Dmin)
        assert D[j] - Dmin <= tol, (s, D[j], Dmin)
        c = near[s]["point"].astype(np.float64)
        lo, hi = cl.voxel_boxes(rows[j:j + 1])
        assert (c >= lo[0]).all() and (c <= hi[0]).all()
        assert abs(((c - p) ** 2).sum() - D[j]) <= 16 * 2.0 ** -53 * D[j]
        checked += 1
    assert checked == cu.N - 7


# ------------------------------------------------------------------------------------ header == model
@pytest.mark.parametrize("name,coarse,unbounded", CASES)
def test_driver_equals_model(driver, name, coarse, unbounded):
    svo, _ = gm.pool(name)
    queries, _ = cu.batch(name)
    want, want_con, _ = cu.model(name, unbounded, coarse)
    got, got_con = driver(svo, queries, flags=1 if unbounded else 0, coarse_level=coarse)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:8]
    assert got_con.tobytes() == want_con.tobytes()
    if coarse:
        plain = cu.model(name, unbounded, 0)[0]
        assert (want["visits"] <= plain["visits"]).all() and (want["d2"] <= plain["d2"]).all()
        assert (want["visits"] < plain["visits"]).sum() >= 20


def test_budget_and_guard_pools(driver):
    """The walk ends on a budget, on a cycle and on an over-deep pool, and the header says what the model says."""
    svo, _ = gm.pool("walk7")
    far = cl.make_queries([[1.0e30, 0.0, 0.0], [0.0, 0.0, 0.0]], 1.0)      # every d2 is +inf: every tie is entered
    full, _, _ = cl.closest_model(svo, far, flags=cl.CLOSEST_UNBOUNDED)
    assert full["visits"][0] == np.count_nonzero(svo.levels() > 0) and full["flags"][0] == 1
    n, c, _ = cl.closest_model(svo, far, flags=cl.CLOSEST_UNBOUNDED, max_visits=100)
    assert n["visits"][0] == 100 and n["flags"][0] == (cl.FLAG_FOUND | cl.FLAG_BUDGET) and np.isinf(n["d2"][0])
    assert n[1].tobytes() == full[1].tobytes() and full["visits"][1] < 100
    gn, gc = driver(svo, far, flags=1, max_visits=100)
    assert gn.tobytes() == n.tobytes() and gc.tobytes() == c.tobytes()
    n, c, _ = cl.closest_model(svo, far, flags=cl.CLOSEST_UNBOUNDED, max_visits=3)
    assert (n["visits"] == 3).all() and (n["flags"] == cl.FLAG_BUDGET).all(), "ended before the first voxel: nothing found"
    gn, gc = driver(svo, far, flags=1, max_visits=3)
    assert gn.tobytes() == n.tobytes() and gc.tobytes() == c.tobytes()
    for name in ("cyclic7", "layered24"):
        pool = guard_svo(name)
        for flags in (0, cl.CLOSEST_UNBOUNDED):
            n, c, _ = cl.closest_model(pool, cu.GUARD_QUERIES, flags=flags, max_visits=1000)
            assert (n["visits"] <= 1000).all() and (n["flags"] & cl.FLAG_OVERFLOW).any(), "the corner query reaches level 22"
            assert n["flags"][0] & 1 and n["flags"][1] & 1
            if name == "cyclic7" and flags:
                assert n["flags"][3] & cl.FLAG_BUDGET and n["visits"][3] == 1000
            gn, gc = driver(pool, cu.GUARD_QUERIES, flags=flags, max_visits=1000)
            assert gn.tobytes() == n.tobytes() and gc.tobytes() == c.tobytes()


def test_driver_under_sanitizers(tmp_path, driver):
    """The header's walk under AddressSanitizer and UBSan on the host, as a program of its own: the guard pools
    reach every stack level, the tree batch every branch of the pick."""
    exe = tmp_path / "closest_driver_san"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "closest_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-400:]
    for name in ("cyclic7", "layered24"):
        svo = guard_svo(name)
        n, c, _ = cl.closest_model(svo, cu.GUARD_QUERIES, flags=cl.CLOSEST_UNBOUNDED, max_visits=1000)
        gn, gc = driver(svo, cu.GUARD_QUERIES, flags=1, max_visits=1000, exe=exe)
        assert gn.tobytes() == n.tobytes() and gc.tobytes() == c.tobytes()
    want, want_con, _ = cu.model("mixed", True, 11)
    gn, gc = driver(gm.pool("mixed")[0], cu.batch("mixed")[0], flags=1, coarse_level=11, exe=exe)
    assert gn.tobytes() == want.tobytes() and gc.tobytes() == want_con.tobytes()


def test_c_example_compiles_and_links(tmp_path):
    from tests.test_c_host import _build
    assert os.path.exists(_build(tmp_path, os.path.join(ROOT, "examples", "closest_min.c"), "closest_min"))


def test_object_queries_is_the_object_rule_on_a_point():
    """closest.object_queries is overlap.object_spheres: the point moves as a ray origin does, the radius scales."""
    ob = np.zeros(1, _lib.OBJECT_DTYPE)
    a = 0.4
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]], np.float32)
    ob["root"], ob["scale_log2"], ob["position"], ob["rotation"] = 64, -1, (1.0, 2.0, -3.5), R.reshape(-1)
    pts = np.random.default_rng(9).uniform(-20.0, 20.0, (32, 3)).astype(np.float32)
    got = cl.object_queries(pts, 0.5, ob[0])
    assert got.tobytes() == ov.object_spheres(pts, 0.5, ob[0]).tobytes()
    assert (got["kind"] == 1).all() and (got["q"][:, 0] == np.float32(1.0)).all() and cl.queries_valid(got).all()
