"""Volume queries without a GPU: the rule's header (csrc/svo_overlap.h, built by plain g++ into
tests/overlap_driver.cpp) against its Python statement (overlap.overlap_model) byte for byte, the model against a
brute force over all leaves (overlap.overlap_bruteforce), conditions on the batch so that no test passes on
degenerate inputs, and the C API's argument errors from the loaded library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from raytracingtest_amd import _lib
from raytracingtest_amd import overlap as ov
from raytracingtest_amd.svo_data import SVOData
from tests import geometry_model as gm
from tests import guard_pools
from tests import overlap_util as ou
from tests.conftest import ROOT

NAMES = ("svo_overlap_volumes", "svo_overlap_volumes_host")


@pytest.fixture(scope="module")
def native():
    from raytracingtest_amd import build
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("overlap") / "overlap_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "overlap_driver.cpp"), "-o", str(exe)], check=True)

    def run(svo, shapes, root=0, K=0, flags=0, max_visits=0, coarse_level=0, exe=exe):
        d = tmp_path_factory.mktemp("run")
        svo.to_v2().astype("<u8").tofile(d / "nodes.bin")
        np.ascontiguousarray(shapes, ov.SHAPE_DTYPE).tofile(d / "shapes.bin")
        subprocess.run([str(exe), str(d / "nodes.bin"), str(d / "shapes.bin"), str(d / "summary.bin"), str(d / "contacts.bin"),
                        str(root), str(K), str(flags), str(max_visits), str(coarse_level)], check=True)
        return (np.fromfile(d / "summary.bin", ov.OVERLAP_DTYPE),
                np.fromfile(d / "contacts.bin", ov.CONTACT_DTYPE).reshape(len(shapes), K))
    return run


# ------------------------------------------------------------------------------------ the surface
def test_symbols_layouts_and_abi(native, tmp_path):
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(native, name)
    assert native.svo_abi_version() == _lib.ABI_VERSION == 10
    src = tmp_path / "t.c"
    src.write_text('#include "svo_rt.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(svo_shape) == 32 && offsetof(svo_shape, kind) == 12 && offsetof(svo_shape, q) == 16, "shape");\n'
                   '_Static_assert(sizeof(svo_contact) == 16 && offsetof(svo_contact, key) == 8, "contact");\n'
                   '_Static_assert(sizeof(svo_overlap) == 16 && offsetof(svo_overlap, flags) == 8, "summary");\n'
                   '_Static_assert(sizeof(svo_overlap_params) == 24 && offsetof(svo_overlap_params, coarse_level) == 20, "params");\n'
                   '_Static_assert(sizeof(svo_overlap_out) == 3 * sizeof(void *), "out");\n'
                   '_Static_assert(SVO_SHAPE_BOX == 0 && SVO_SHAPE_SPHERE == 1 && SVO_OVERLAP_ANY == 1, "enums");\n'
                   'int main(void){return 0;}\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "t")], check=True)
    assert ctypes.sizeof(_lib.SvoOverlapParams) == 24 and ctypes.sizeof(_lib.SvoOverlapOut) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert ov.SHAPE_DTYPE.fields["kind"][1] == 12 and ov.CONTACT_DTYPE.fields["key"][1] == 8


def test_csharp_shim_declares_the_calls():
    text = open(os.path.join(ROOT, "unity", "RaytracingMasterNative.cs")).read()
    for name in NAMES:
        assert re.search(rf"\[DllImport\(Lib\)\] public static extern int {name}\(", text), name
    assert "public int OverlapVolumes(" in text
    # no C# toolchain here: each struct has the header's fields, in order, as 4-byte words (ulong: 8)
    for struct, words in (("SvoShape", 8), ("SvoContact", 4), ("SvoOverlap", 4), ("SvoOverlapParams", 6)):
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
    shapes, summary, contacts, mask = base, base + 1024, base + 2048, base + 3072
    P = _lib.overlap_params
    out = lambda s=summary, c=None, m=None: ctypes.byref(_lib.SvoOverlapOut(s, c, m))   # noqa: E731

    def dev(ctx_=ctx, shapes_=shapes, n=4, prm=P(), out_=None):
        return native.svo_overlap_volumes(ctx_, shapes_, n, ctypes.byref(prm) if prm is not None else None,
                                          out() if out_ is None else out_, None)

    def host(ctx_=ctx, shapes_=shapes, n=4, prm=P(), summary_=summary, contacts_=None):
        return native.svo_overlap_volumes_host(ctx_, shapes_, n, ctypes.byref(prm) if prm is not None else None, summary_,
                                               contacts_)

    def err():
        return native.svo_last_error().decode()

    assert dev(ctx_=None) == -1 and "null context" in err()
    assert dev(shapes_=None) == -1 and "null shape list" in err()
    assert native.svo_overlap_volumes(ctx, shapes, 4, ctypes.byref(P()), None, None) == -1 and "null svo_overlap_out" in err()
    assert dev(out_=out(None, None, None)) == -1 and "every overlap output is null" in err()
    assert host(ctx_=None) == -1 and host(shapes_=None) == -1
    assert host(summary_=None) == -1 and "every overlap output is null" in err()
    for call in (dev, host):
        assert call(prm=P(any_hit=True)) == -1 and "root" in err()     # a good flag passes the flag test
        bad = P()
        bad.flags = 2
        assert call(prm=bad) == -1 and "unknown overlap flag bits" in err()
        assert call(prm=P(max_contacts=33)) == -1 and "max_contacts" in err()
        assert call(prm=P(max_visits=(1 << 24) + 1)) == -1 and "max_visits" in err()
        assert call(prm=P(coarse_level=23)) == -1 and "coarse_level" in err()
        small = P()
        small.size = 4
        assert call(prm=small) == -1 and "size" in err()
        big = P()
        big.size = 28
        assert call(prm=big) == -1 and "newer ABI" in err()
        # root >= capacity: the fake context's capacity is 0, so every root is outside
        assert call(prm=P(root=0)) == -1 and "root outside the node-pool capacity" in err()
        assert call(prm=None) == -1 and "root outside the node-pool capacity" in err()   # NULL params: the defaults
    assert dev(prm=P(max_contacts=0), out_=out(summary, contacts, None)) == -1 and "max_contacts 0" in err()
    assert host(prm=P(max_contacts=0), contacts_=contacts) == -1 and "max_contacts 0" in err()
    assert bytes(fake) == bytes(1 << 20) and not raw.any()


def test_count_limits_without_a_gpu(native):
    """n and n K above 2^31 - 1: the count tests stand before the root test, so the zeroed context shows them; the
    largest counts that pass them end at the root test (capacity 0), not at a device."""
    fake = ctypes.create_string_buffer(1 << 20)
    ctx = ctypes.addressof(fake)
    raw = np.zeros(256, np.uint8)
    shapes = raw.ctypes.data + (-raw.ctypes.data % 16)
    P = _lib.overlap_params
    host = lambda n, prm: native.svo_overlap_volumes_host(ctx, shapes, n, ctypes.byref(prm), shapes + 64, None)   # noqa: E731
    assert host(1 << 31, P()) == -1 and b"2^31 - 1 shapes" in native.svo_last_error()
    assert host((1 << 31) - 1, P()) == -1 and b"root outside" in native.svo_last_error()
    assert host(1 << 27, P(max_contacts=16)) == -1 and b"2^31 - 1 contacts" in native.svo_last_error()
    assert host((1 << 27) - 1, P(max_contacts=16)) == -1 and b"root outside" in native.svo_last_error()
    out = _lib.SvoOverlapOut(shapes + 64, None, None)
    assert native.svo_overlap_volumes(ctx, shapes, 1 << 31, ctypes.byref(P()), ctypes.byref(out), None) == -1
    assert b"2^31 - 1 shapes" in native.svo_last_error()
    assert bytes(fake) == bytes(1 << 20) and not raw.any()


# ------------------------------------------------------------------------------------ the batch
@pytest.mark.parametrize("name", ou.POOLS)
def test_batch_conditions(name):
    """The batch is what its docstring says: counts above 32 and of 0, closedness and exact spheres decide."""
    svo, leaves = gm.pool(name)
    shapes, parts = ou.batch(name)
    summary, contacts, mask = ou.model(name)
    count = summary["count"].astype(np.int64)
    assert 800 <= len(leaves) <= 2000   # walk7 1,4xx; mixed fewer, a third of its level-10 / 11 descriptors being leaves
    assert (count[parts["whole"]][[0, 1, 3, 4]] == len(leaves)).all() and 0 < count[parts["whole"]][2] < len(leaves)
    assert (count[parts["outside"]] == 0).all() and (summary["visits"][parts["outside"]] == 1).all()
    assert (count[parts["face"]] >= 1).all(), "a box sharing a face plane with a leaf touches it"
    pt = count[parts["point"]]
    assert (pt[:9] >= 1).all() and (pt[9:15] == 1).all()
    ex = count[parts["exact"]]
    assert (ex[0::2] >= 1).all() and (ex[0::2] > ex[1::2]).sum() >= 6, "d2 == r r touches, the next smaller radius does not"
    assert (count[parts["zero"]][:3] >= 1).all() and (count[parts["zero"]][3:] == 0).all()
    assert (summary["flags"][parts["invalid"]] == ov.FLAG_INVALID).all() and (count[parts["invalid"]] == 0).all()
    assert (count > 32).sum() >= 8 and (count == 0).sum() >= 20 and ((count > 0) & (count <= 8)).sum() >= 40
    assert set(np.unique(shapes["kind"])) == {0, 1, 7}


@pytest.mark.parametrize("name", ou.POOLS)
def test_model_equals_bruteforce_and_visits(name):
    """Pruning equals brute force; at the default budget nothing on these pools carries the budget or the overflow
    flag.  Visits: every valid shape fetches the root; the whole-cube volumes fetch every descriptor exactly once;
    a point in the middle of a leaf at level L walks one path, L descriptors; nothing fetches more than the tree has."""
    svo, leaves = gm.pool(name)
    shapes, parts = ou.batch(name)
    summary, contacts, mask = ou.model(name)
    assert not (summary["flags"] & (ov.FLAG_BUDGET | ov.FLAG_OVERFLOW)).any()
    brute = ov.overlap_bruteforce(leaves, shapes)
    assert (summary["count"] == brute).all(), np.flatnonzero(summary["count"] != brute)[:8]
    assert ((summary["flags"] & 1) == (brute > 0)).all()
    reachable = int(np.count_nonzero(svo.levels() > 0))
    valid = ov.shapes_valid(shapes)
    assert (summary["visits"][valid] >= 1).all() and (summary["visits"][~valid] == 0).all()
    assert (summary["visits"] <= reachable).all()
    assert (summary["visits"][parts["whole"]][[0, 1, 3, 4]] == reachable).all()
    mid = np.arange(N_POINT_MID.start, N_POINT_MID.stop) + parts["point"].start
    for s in mid:
        row = leaves[(leaves[:, 0] == contacts[s, 0]["parent"]) & (leaves[:, 1] == (contacts[s, 0]["meta"] & 0xFF))]
        assert len(row) == 1 and summary["visits"][s] == row[0, 2]
    # contacts: walk order is Morton order of the leaves, each a leaf of the pool with its key
    keys = {(int(r[0]), int(r[1])): (int(r[2]), int(k)) for r, k in zip(leaves, gm.voxel_keys(leaves))}
    for s in np.flatnonzero(summary["count"] > 0):
        k = min(int(summary["count"][s]), 32)
        got = contacts[s, :k]
        for c in got:
            level, key = keys[(int(c["parent"]), int(c["meta"] & 0xFF))]
            assert (c["meta"] >> 8) == 23 - level and int(c["key"]) == key
        assert (contacts[s, k:]["parent"] == 0xFFFFFFFF).all()
        assert morton_sorted(got)
    want_mask = np.zeros_like(mask)
    for s in np.flatnonzero(brute > 0):
        want_mask[s // 64] |= np.uint64(1 << (s % 64))
    assert (mask == want_mask).all()


N_POINT_MID = slice(9, 15)   # the points in leaf centres within the batch's "point" part


def morton_sorted(contacts):
    """Walk order: the voxels' corners, refined to the finest level, ascend in z-y-x interleaved order."""
    codes = []
    for c in contacts:
        level = 23 - (int(c["meta"]) >> 8)
        xyz = [(int(c["key"]) >> (21 * k)) & 0x1FFFFF for k in range(3)]
        code = 0
        for b in range(level - 1, -1, -1):
            code = code << 3 | ((xyz[2] >> b) & 1) << 2 | ((xyz[1] >> b) & 1) << 1 | ((xyz[0] >> b) & 1)
        codes.append(code << (3 * (22 - level)))
    return all(a < b for a, b in zip(codes, codes[1:]))


# ------------------------------------------------------------------------------------ header == model
@pytest.mark.parametrize("name,any_hit,coarse", [("walk7", False, 0), ("walk7", True, 0), ("mixed", False, 0),
                                                 ("mixed", True, 0), ("mixed", False, 9), ("mixed", False, 11),
                                                 ("mixed", True, 11)])
def test_driver_equals_model(driver, name, any_hit, coarse):
    svo, _ = gm.pool(name)
    shapes, _ = ou.batch(name)
    for K in (0, 1, 8, 32):
        want_s, want_c, _ = ou.expected(name, K, any_hit, coarse)
        got_s, got_c = driver(svo, shapes, K=K, flags=1 if any_hit else 0, coarse_level=coarse)
        assert got_s.tobytes() == want_s.tobytes(), np.flatnonzero(got_s != want_s)[:8]
        assert got_c.tobytes() == want_c.tobytes(), np.flatnonzero((got_c != want_c).any(axis=1))[:8]
    if any_hit:
        assert (want_s["count"] <= 1).all() and (want_s["count"] == 1).sum() >= 100
    if coarse:
        plain = ou.model(name)[0]
        # a touched coarse voxel need not hold a touched leaf, so the counts are not ordered shape by shape
        assert (want_s["count"] != plain["count"]).sum() >= 10 and (want_s["count"][:2] < plain["count"][:2]).all()
        assert ((want_s["count"] > 0) >= (plain["count"] > 0)).all()
        assert (want_s["visits"] <= plain["visits"]).all()


def guard_svo(name):
    nodes, att = guard_pools.POOLS[name]()
    return SVOData(nodes=nodes, attachments=att)


GUARD_SHAPES = np.concatenate([ov.make_boxes([[-16.0] * 3, [-16.0, -16.0, -16.0], [3.0, 3.0, 3.0]],
                                             [[16.0] * 3, [-15.0, -15.0, -15.0], [3.5, 3.25, 4.0]]),
                               ov.make_spheres([[0.0, 0.0, 0.0], [-16.0, -16.0, -16.0]], [40.0, 2.0 ** -12])])


def test_budget_and_guard_pools(driver):
    """The walk ends on a budget, on a cycle and on an over-deep pool, and the header says what the model says."""
    svo, _ = gm.pool("walk7")
    whole = ov.make_boxes([[-16.0] * 3], [[16.0] * 3])
    s, c, _ = ov.overlap_model(svo, whole, max_contacts=8, max_visits=50)
    assert s["visits"][0] == 50 and s["flags"][0] & ov.FLAG_BUDGET and 0 < s["count"][0] < ou.model("walk7")[0]["count"][0]
    gs, gc = driver(svo, whole, K=8, max_visits=50)
    assert gs.tobytes() == s.tobytes() and gc.tobytes() == c.tobytes()
    cyc = guard_svo("cyclic7")
    s, c, _ = ov.overlap_model(cyc, GUARD_SHAPES, max_contacts=8, max_visits=1000)
    assert (s["flags"][[0, 3]] & ov.FLAG_BUDGET).all() and (s["visits"] <= 1000).all()
    assert (s["flags"] & ov.FLAG_OVERFLOW).any(), "a small volume in the cycle's corner reaches level 22"
    gs, gc = driver(cyc, GUARD_SHAPES, K=8, max_visits=1000)
    assert gs.tobytes() == s.tobytes() and gc.tobytes() == c.tobytes()
    deep = guard_svo("layered24")
    s, c, _ = ov.overlap_model(deep, GUARD_SHAPES, max_contacts=8, max_visits=1000)
    assert (s["flags"] & ov.FLAG_OVERFLOW).any() and (s["visits"] <= 1000).all()
    gs, gc = driver(deep, GUARD_SHAPES, K=8, max_visits=1000)
    assert gs.tobytes() == s.tobytes() and gc.tobytes() == c.tobytes()


def test_driver_under_sanitizers(tmp_path, driver):
    """The header's walk under AddressSanitizer and UBSan on the host: the guard pools reach every stack level."""
    exe = tmp_path / "overlap_driver_san"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "overlap_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-400:]
    for name in ("cyclic7", "layered24"):
        svo = guard_svo(name)
        s, c, _ = ov.overlap_model(svo, GUARD_SHAPES, max_contacts=32, max_visits=1000)
        gs, gc = driver(svo, GUARD_SHAPES, K=32, max_visits=1000, exe=exe)
        assert gs.tobytes() == s.tobytes() and gc.tobytes() == c.tobytes()


def test_c_example_compiles_and_links(tmp_path):
    from tests.test_c_host import _build
    assert os.path.exists(_build(tmp_path, os.path.join(ROOT, "examples", "overlap_min.c"), "overlap_min"))


def test_object_spheres_is_the_object_rule_on_a_point():
    """overlap.object_spheres against objects.object_rays: the centre moves as a ray origin does, the radius scales."""
    from raytracingtest_amd import objects as obj_rule
    from raytracingtest_amd.query import make_rays
    rng = np.random.default_rng(5)
    a = 0.7
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]], np.float32)
    ob = np.zeros(1, _lib.OBJECT_DTYPE)
    ob["root"], ob["scale_log2"], ob["position"], ob["rotation"] = 100, -2, (3.0, -1.5, 8.25), R.reshape(-1)
    c = rng.uniform(-20.0, 20.0, (64, 3)).astype(np.float32)
    r = rng.uniform(0.1, 4.0, 64).astype(np.float32)
    got = ov.object_spheres(c, r, ob[0])
    rays = obj_rule.object_rays(make_rays(c, np.tile([1.0, 0.0, 0.0], (64, 1)), np.inf), ob[0])
    assert got["p"].tobytes() == rays["origin"].tobytes()
    assert (got["q"][:, 0] == r * np.float32(4.0)).all() and (got["kind"] == 1).all()
