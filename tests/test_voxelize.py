"""Meshes without a GPU: the surface of svob_build_mesh / svob_mesh_leaves, the rule's header
(csrc/svo_voxelize.h through plain g++, tests/voxelize_driver.cpp) against its numpy statement (voxelize.py) bit
for bit, the numpy statement against an independent float64 separating-axis model (tests/voxelize_util.py), the
owner and attribute rules, and a watertightness check through the CPU oracle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from raytracingtest_amd import builder
from raytracingtest_amd import native_builder as nb
from raytracingtest_amd import voxelize as vz
from raytracingtest_amd.query import make_rays
from tests import query_util as qu
from tests import voxelize_util as vu
from tests.conftest import ROOT

f32 = np.float32
FUNCS = ("svob_build_mesh", "svob_mesh_leaves")


@pytest.fixture(scope="module")
def native():
    from raytracingtest_amd import build
    build.build()
    return nb.blib()


# ------------------------------------------------------------------ 1. the surface
def test_exports_present(native):
    header = open(os.path.join(ROOT, "include", "svo_build.h")).read()
    for name in FUNCS:
        assert hasattr(native, name)
        assert re.search(rf"\bint {name}\s*\(", header), name
    assert re.search(r"enum \{ SVOB_MESH_FLIP_WINDING = 1 \};", header) and nb.MESH_FLIP_WINDING == 1
    assert callable(nb.build_mesh_svo) and callable(nb.mesh_leaves)


def test_header_compiles_in_c_and_matches_ctypes(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include <stddef.h>\n#include "svo_build.h"\n'
                   'int (*a)(int, const svob_mesh *, int, const svob_limits *, svob_report *, svob_mesh_stats *,'
                   ' svob_result *) = svob_build_mesh;\n'
                   'int (*b)(int, const svob_mesh *, int, const svob_limits *, svob_report *, svob_mesh_stats *, size_t *,'
                   ' uint64_t **, float **, float **, uint32_t **) = svob_mesh_leaves;\n'
                   '_Static_assert(sizeof(svob_mesh) == 48 && offsetof(svob_mesh, flags) == 4 &&'
                   ' offsetof(svob_mesh, positions) == 8 && offsetof(svob_mesh, n_vertices) == 16 &&'
                   ' offsetof(svob_mesh, indices) == 24 && offsetof(svob_mesh, n_triangles) == 32 &&'
                   ' offsetof(svob_mesh, colors) == 40, "svob_mesh layout");\n'
                   '_Static_assert(sizeof(svob_mesh_stats) == 40 && offsetof(svob_mesh_stats, degenerate) == 8 &&'
                   ' offsetof(svob_mesh_stats, outside) == 16 && offsetof(svob_mesh_stats, candidates) == 24 &&'
                   ' offsetof(svob_mesh_stats, overlaps) == 32, "svob_mesh_stats layout");\n'
                   '_Static_assert(SVOB_MESH_FLIP_WINDING == 1, "flag");\n'
                   '_Static_assert(sizeof(svob_limits) == 40 && offsetof(svob_limits, max_blocks) == 28 &&'
                   ' offsetof(svob_limits, launch_candidates) == 32, "svob_limits: the older fields stay, one appended");\n'
                   '_Static_assert(sizeof(svob_report) == 40 && offsetof(svob_report, list_capacity) == 24 &&'
                   ' offsetof(svob_report, overlap_launches) == 32, "svob_report: the older fields stay, one appended");\n'
                   'int main(void){return 0;}\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "a.o")], check=True)
    M, S = nb._Mesh, nb._MeshStats
    assert ctypes.sizeof(M) == 48 and ctypes.sizeof(S) == 40
    assert [getattr(M, k).offset for k in ("size", "flags", "positions", "n_vertices", "indices", "n_triangles",
                                           "colors")] == [0, 4, 8, 16, 24, 32, 40]
    assert [getattr(S, k).offset for k in ("size", "reserved", "degenerate", "outside", "candidates", "overlaps")] == \
        [0, 4, 8, 16, 24, 32]
    assert ctypes.sizeof(nb._Limits) == 40 and nb._Limits.max_blocks.offset == 28 and nb._Limits.launch_candidates.offset == 32
    assert ctypes.sizeof(nb._Report) == 40 and nb._Report.list_capacity.offset == 24 and nb._Report.overlap_launches.offset == 32
    assert "launch_candidates" in nb.LIMIT_FIELDS and nb.MESH_REPORT_FIELDS == nb.REPORT_FIELDS + ("overlap_launches",)


def _call(native, mesh, max_level=5, limits=None, stats=None, report=None):
    res = nb._Result()
    return native.svob_build_mesh(0, None if mesh is None else ctypes.byref(mesh), max_level, limits,
                                  None if report is None else ctypes.byref(report),
                                  None if stats is None else ctypes.byref(stats), ctypes.byref(res)), res


def _raw_mesh(pos, tri, col=None, flags=0):
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    m = nb._Mesh(size=ctypes.sizeof(nb._Mesh), flags=flags, positions=pos.ctypes.data, n_vertices=len(pos),
                 indices=tri.ctypes.data, n_triangles=len(tri), colors=None if col is None else col.ctypes.data)
    return m, (pos, tri, col)


GOOD_POS = np.array([(0.2, 0.2, 0.2), (0.7, 0.3, 0.2), (0.3, 0.8, 0.6)], f32)


def test_arguments_rejected_without_gpu(native):
    """Every refusal comes back as -1 (argument), never as a HIP error: no device is touched."""
    def refused(rc, word):
        assert rc == -1, (rc, native.svob_last_error())
        assert word.encode() in native.svob_last_error(), native.svob_last_error()

    m, keep = _raw_mesh(GOOD_POS, [(0, 1, 2)])
    refused(_call(native, None)[0], "null mesh")
    assert native.svob_build_mesh(0, ctypes.byref(m), 5, None, None, None, None) == -1
    for bad in (1, 23, -4):
        refused(_call(native, m, max_level=bad)[0], "max_level")
    refused(_call(native, _raw_mesh(GOOD_POS, [(0, 1, 3)])[0])[0], "names vertex 3")
    for value in (np.nan, np.inf, -np.inf):
        p = GOOD_POS.copy()
        p[1, 2] = value
        m2, keep2 = _raw_mesh(p, [(0, 1, 2)])
        refused(_call(native, m2)[0], "vertex 1 is not finite")
    m3, keep3 = _raw_mesh(GOOD_POS, [(0, 1, 2)], flags=2)
    refused(_call(native, m3)[0], "flags")
    m4, keep4 = _raw_mesh(GOOD_POS, [(0, 1, 2)])
    m4.positions = None
    refused(_call(native, m4)[0], "positions is null")
    m5, keep5 = _raw_mesh(GOOD_POS, [(0, 1, 2)])
    m5.indices = None
    refused(_call(native, m5)[0], "indices is null")
    m6, keep6 = _raw_mesh(GOOD_POS, [(0, 1, 2)])
    m6.n_triangles = 0xFFFFFFFF
    refused(_call(native, m6)[0], "n_triangles")
    # a grid of which the budget does not hold one plane: refused, not over-allocated
    refused(_call(native, m, max_level=15)[0], "one plane")
    lim = nb._Limits(size=ctypes.sizeof(nb._Limits), cell_bytes=4 * 16 * 16 - 1)
    refused(_call(native, m, max_level=5, limits=ctypes.byref(lim))[0], "one plane")
    st = nb._MeshStats(size=2)
    refused(_call(native, m, stats=st)[0], "svob_mesh_stats.size")
    # svob_mesh_leaves: the same checks, and its own outputs
    n, p = ctypes.c_size_t(), [ctypes.c_void_p() for _ in range(4)]
    rc = native.svob_mesh_leaves(0, None, 5, None, None, None, ctypes.byref(n), *[ctypes.byref(q) for q in p])
    refused(rc, "null mesh")
    assert native.svob_mesh_leaves(0, ctypes.byref(m), 5, None, None, None, None, *[ctypes.byref(q) for q in p]) == -1
    with pytest.raises(nb.SvoError):
        nb.mesh_leaves(GOOD_POS, [(0, 1, 2)], 5, colors=np.zeros((2, 3), f32))


def test_mesh_struct_is_versioned_by_size(native):
    """svob_mesh like svob_limits: a size below the header or above the library's is refused, a shorter struct is
    read up to its size and the rest is zero.  A mesh without triangles launches nothing, so the accepted cases
    return an empty tree here, without a GPU."""
    bad_pos = GOOD_POS.copy()
    bad_pos[0, 0] = np.nan
    m, keep = _raw_mesh(bad_pos, [(0, 1, 7)])
    for size in (0, 4, ctypes.sizeof(nb._Mesh) + 8):
        m.size = size
        assert _call(native, m)[0] == -1 and b"svob_mesh.size" in native.svob_last_error()
    m.size = ctypes.sizeof(nb._Mesh)
    assert _call(native, m)[0] == -1
    m.size = nb._Mesh.indices.offset          # positions and n_vertices are read: the NaN is seen, the index is not
    assert _call(native, m)[0] == -1 and b"not finite" in native.svob_last_error()
    m.size = 8                                # nothing but the header: an empty mesh
    st = nb._MeshStats(size=ctypes.sizeof(nb._MeshStats), degenerate=7, outside=7, candidates=7, overlaps=7)
    rep = nb._new_report()
    rc, res = _call(native, m, stats=st, report=rep)
    assert rc == 0, native.svob_last_error()
    assert res.n_nodes == 1 and res.n_leaves == 0 and res.depth == 4 and res.nodes[0] == 0
    assert nb._stats_dict(st) == {"degenerate": 0, "outside": 0, "candidates": 0, "overlaps": 0}
    assert rep.slabs == 0 and rep.slab_rows == 16
    native.svob_free(ctypes.byref(res))
    good, keep2 = _raw_mesh(GOOD_POS, [(0, 1, 7)])
    good.size = nb._Mesh.indices.offset       # the bad index lies past the caller's size
    rc, res = _call(native, good)
    assert rc == 0 and res.n_leaves == 0
    native.svob_free(ctypes.byref(res))
    # svob_mesh_stats: at most `size` bytes are written
    st = nb._MeshStats(size=16, degenerate=7, outside=7, candidates=7, overlaps=7)
    rc, res = _call(native, m, stats=st)
    assert rc == 0 and (st.size, st.degenerate, st.outside, st.candidates, st.overlaps) == (16, 0, 7, 7, 7)
    native.svob_free(ctypes.byref(res))
    # the empty mesh through the bindings
    codes, nrm, col, owner = nb.mesh_leaves(np.zeros((0, 3), f32), np.zeros((0, 3), np.uint32), 5)
    assert len(codes) == 0 and nrm.shape == (0, 3) and col is None and owner.dtype == np.uint32
    svo = nb.build_mesh_svo(np.zeros((0, 3), f32), np.zeros((0, 3), np.uint32), 5)
    ref = nb.build_from_leaves(4, np.zeros((0, 3), np.uint32), np.zeros((0, 3), f32))
    assert svo.format == ref.format == 1 and np.array_equal(svo.childDescriptors, ref.childDescriptors)
    assert np.array_equal(svo.attachments, ref.attachments)


def test_launch_limit_and_report_field_without_gpu(native):
    """svob_limits.launch_candidates takes every value, and svob_report.overlap_launches is written (0: a mesh
    without triangles launches nothing) -- unless the caller's report is the older, shorter struct."""
    m, keep = _raw_mesh(np.zeros((0, 3), f32), np.zeros((0, 3), np.uint32))
    for value in (0, 1, 63, 2 ** 28, 2 ** 64 - 1):
        lim = nb._Limits(size=ctypes.sizeof(nb._Limits), launch_candidates=value)
        rep = nb._new_report()
        rep.overlap_launches = rep.slabs = 7
        rc, res = _call(native, m, limits=ctypes.byref(lim), report=rep)
        assert rc == 0, native.svob_last_error()
        assert (rep.size, rep.slabs, rep.overlap_launches, rep.reserved2) == (ctypes.sizeof(nb._Report), 0, 0, 0)
        native.svob_free(ctypes.byref(res))
    old = nb._Report(size=nb._Report.overlap_launches.offset, slabs=7, overlap_launches=7)
    rc, res = _call(native, m, report=old)
    assert rc == 0 and (old.size, old.slabs, old.overlap_launches) == (32, 0, 7)
    native.svob_free(ctypes.byref(res))
    with pytest.raises(nb.SvoError):
        nb.mesh_leaves(GOOD_POS, [(0, 1, 2)], 5, limits={"launch_candidate": 5})
    out = nb.mesh_leaves(np.zeros((0, 3), f32), np.zeros((0, 3), np.uint32), 5, limits={"launch_candidates": 5}, report=True)
    assert out[4] == {"slabs": 0, "slab_rows": 16, "relaunches": 0, "normals_regrown": 0,
                      "list_capacity": 1 << 20, "overlap_launches": 0}


def test_bindings_declare_meshes():
    text = open(os.path.join(ROOT, "unity", "RaytracingMasterNative.cs")).read()
    assert re.search(r"\[DllImport\(Builder\)\] public static extern int svob_build_mesh\(", text)
    assert re.search(r"public struct SvobMesh \{", text) and re.search(r"public struct SvobMeshStats \{", text)
    assert re.search(r"public ulong SetSVOFromMesh\(Mesh mesh, int maxLevel, ulong dstOffset\)", text)
    assert re.search(r"svob_build_mesh\(0, ref m, maxLevel,", text)
    assert "oracle" not in open(os.path.join(ROOT, "raytracingtest_amd", "voxelize.py")).read()


def test_mesh_min_example_compiles(tmp_path):
    from tests.test_c_host import _build
    exe = _build(tmp_path, os.path.join(ROOT, "examples", "mesh_min.c"), "mesh_min", ("-lsvo_rt", "-lsvo_build"))
    assert os.path.exists(exe)


# ------------------------------------------------------------------ 2. the rule: header against numpy
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("voxelize") / "voxelize_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "voxelize_driver.cpp"), "-o", str(exe)], check=True)
    return exe


def run_driver(exe, pos, tri, depth, col=None, flip=False):
    d = exe.parent
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([len(pos), len(tri), depth, (1 if col is not None else 0) | (2 if flip else 0)], np.uint32).tobytes())
        f.write(np.ascontiguousarray(pos, f32).tobytes())
        f.write(np.ascontiguousarray(tri, np.uint32).tobytes())
        if col is not None:
            f.write(np.ascontiguousarray(col, f32).tobytes())
    subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], check=True)
    raw = (d / "out.bin").read_bytes()
    head = np.frombuffer(raw, np.uint64, 5)
    m = int(head[0])
    at = 40
    codes = np.frombuffer(raw, np.uint64, m, at)
    at += 8 * m
    owner = np.frombuffer(raw, np.uint32, m, at)
    at += 4 * m
    nrm = np.frombuffer(raw, f32, 3 * m, at).reshape(m, 3)
    at += 12 * m
    leafcol = np.frombuffer(raw, f32, 3 * m, at).reshape(m, 3) if col is not None else None
    assert at + (12 * m if col is not None else 0) == len(raw)
    stats = dict(zip(("degenerate", "outside", "candidates", "overlaps"), (int(v) for v in head[1:])))
    return codes, nrm, leafcol, owner, stats


def same_leaves(got, want, what):
    """codes, normals, colours and owners equal bit for bit (floats compared as words)."""
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[3], want[3]), what
    assert got[1].tobytes() == want[1].tobytes(), what
    assert (got[2] is None) == (want[2] is None), what
    if want[2] is not None:
        assert got[2].tobytes() == want[2].tobytes(), what


@pytest.mark.parametrize("name", vu.MAIN + vu.MORE + vu.EDGES)
def test_header_equals_numpy(driver, name):
    pos, tri, depth = vu.mesh(name)
    want = vu.reference(name)
    got = run_driver(driver, pos, tri, depth, vu.vertex_colors(pos))
    same_leaves(got, want, name)
    assert got[4] == want[4], name
    assert np.array_equal(want[0], np.unique(want[0])) and want[0].dtype == np.uint64
    if name in ("ico2", "all_edges"):   # the winding flag and the colourless form
        same_leaves(run_driver(driver, pos, tri, depth, None, flip=True), vu.reference(name, colors=False, flip=True), name)


def test_driver_under_sanitizers(tmp_path):
    """The stand-alone driver built with -fsanitize=address,undefined runs the edge cases (boxes clipped at every
    face of the grid, skipped triangles) and the soup clean on the CPU, with the same leaves."""
    exe = tmp_path / "voxelize_driver_san"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "voxelize_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-400:]
    for name in ("all_edges", "soup", "empty"):
        pos, tri, depth = vu.mesh(name)
        same_leaves(run_driver(exe, pos, tri, depth, vu.vertex_colors(pos)), vu.reference(name), name)
    cases = decode_cases()
    assert np.array_equal(run_decode(exe, cases)[:, :3], decode_expected(cases))


# ------------------------------------------------------------------ 2b. the candidate decode
def run_decode(exe, cases):
    """The driver's --decode mode on cases [(local, bx, by)]: uint32 [m, 9] = candidate_voxel's, the 64-bit
    form's and (where it applies) the 32-bit form's (x, y, z)."""
    d = exe.parent
    with open(d / "decode_in.bin", "wb") as f:
        f.write(np.array([len(cases)], np.uint64).tobytes())
        f.write(np.array(cases, np.uint64).reshape(-1, 3).tobytes())
    subprocess.run([str(exe), "--decode", str(d / "decode_in.bin"), str(d / "decode_out.bin")], check=True)
    return np.fromfile(d / "decode_out.bin", np.uint32).reshape(len(cases), 9)


def decode_cases():
    """(local, bx, by): local at 0, around 2^32, at 2^40 + 12345 and at the last candidate of a box of 1 and of
    2^21 planes, for widths and depths whose plane stays below 2^32 (local alone selects the 64-bit form), and for
    bx = by = 2^20 (the plane selects it)."""
    sides = (1, 2, 3, 511, 512, 65535)
    boxes = [(bx, by) for bx in sides for by in sides] + [(1 << 20, 1 << 20)]
    out = []
    for bx, by in boxes:
        for local in (0, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 12345, bx * by - 1, bx * by * (1 << 21) - 1):
            out.append((local, bx, by))
    return out


def decode_expected(cases):
    """Python integers: x first, then y, then z; z modulo 2^32 (a candidate of a box has z below 2^21)."""
    return np.array([(local % bx, local // bx % by, local // (bx * by) % 2 ** 32) for local, bx, by in cases], np.uint32)


def test_candidate_voxel_equals_python_integers(driver):
    """candidate_voxel (svo_voxelize.h, called by mesh_overlap_kernel) against Python integers.  Both forms are
    evaluated wherever the 32-bit one applies, and agree; the 64-bit form is selected by local alone and by the
    plane alone."""
    cases = decode_cases()
    want = decode_expected(cases)
    got = run_decode(driver, cases)
    narrow = np.array([local < 2 ** 32 and bx * by < 2 ** 32 for local, bx, by in cases])
    by_local = [c for c in cases if c[0] >= 2 ** 32 and c[1] * c[2] < 2 ** 32]
    by_plane = [c for c in cases if c[0] < 2 ** 32 and c[1] * c[2] >= 2 ** 32]
    assert narrow.sum() >= 36 * 3 and len(by_local) >= 36 * 3 and len(by_plane) == 2
    assert max(bx * by for _, bx, by in cases if (bx, by) != (1 << 20, 1 << 20)) < 2 ** 32
    for k, c in enumerate(cases):
        assert got[k, :3].tolist() == want[k].tolist(), (c, got[k].tolist(), want[k].tolist())
        assert got[k, 3:6].tolist() == want[k].tolist(), ("64-bit form", c)
        if narrow[k]:
            assert got[k, 6:].tolist() == want[k].tolist(), ("32-bit form", c)
    # inside a box every coordinate stays inside it: the last candidate of bx x by x 2^21 is its far corner
    last = [k for k, (local, bx, by) in enumerate(cases) if local == bx * by * (1 << 21) - 1]
    assert all(got[k, :3].tolist() == [cases[k][1] - 1, cases[k][2] - 1, (1 << 21) - 1] for k in last) and len(last) == 37


def test_edge_cases_are_what_the_rule_says():
    """Closed boxes and the skip rules, from the numpy statement."""
    n = 16
    codes, nrm, _, owner, st = vu.reference("quad_in_plane")
    xyz = vz.leaf_xyz(codes)
    assert len(codes) == 2 * n * n and set(xyz[:, 2].tolist()) == {4, 5}   # both layers next to z = 5 / 16
    assert np.all(nrm == np.array([0, 0, 1], f32)) and st["overlaps"] > len(codes)   # the diagonal is shared
    codes, _, _, _, st = vu.reference("vertex_on_corner")
    got = {tuple(v) for v in vz.leaf_xyz(codes).tolist()}
    assert {(x, y, z) for x in (2, 3) for y in (3, 4) for z in (4, 5)} <= got   # the 8 voxels that share the corner
    for name, key in (("zero_area", "degenerate"), ("point", "degenerate"), ("outside", "outside")):
        codes, _, _, _, st = vu.reference(name)
        assert len(codes) == 0 and st[key] == 1 and st["candidates"] == 0, name
    codes, _, _, _, st = vu.reference("crossing")
    xyz = vz.leaf_xyz(codes)
    assert len(codes) > 10 and xyz.max() == n - 1 and st["outside"] == 0
    codes, _, _, _, st = vu.reference("touching")
    assert len(codes) > 0 and np.all(vz.leaf_xyz(codes)[:, 0] == n - 1)   # only the cube's face x = 1 is touched
    for name in ("empty", "vertices_only"):
        codes, nrm, col, owner, st = vu.reference(name)
        assert len(codes) == 0 and nrm.shape == (0, 3) and col.shape == (0, 3) and sum(st.values()) == 0
    codes, _, _, owner, st = vu.reference("all_edges")
    assert st["degenerate"] == 2 and st["outside"] == 1 and set(owner.tolist()) == {2, 3, 5, 6, 7, 8}
    with pytest.raises(ValueError):
        vz.voxelize(np.full((3, 3), np.nan, f32), [(0, 1, 2)], 4)
    with pytest.raises(ValueError):
        vz.voxelize(GOOD_POS, [(0, 1, 3)], 4)


# ------------------------------------------------------------------ 3. numpy against the float64 model
@pytest.mark.parametrize("name", vu.MAIN)
def test_rule_brackets_the_float64_overlap(name):
    """must <= leaves <= may, must / may = the float64 13-axis overlap at half extents 1/2 -+ delta, delta the
    header's forward error bound evaluated on this mesh; the undecided band is a condition on the input."""
    pos, tri, depth = vu.mesh(name)
    codes, _, _, owner, _ = vu.reference(name)
    delta = vu.rule_delta(pos, tri, depth)
    assert 0 < delta <= 1e-3, delta
    must, may = vu.sat_overlap(pos, tri, depth, 0.5 - delta), vu.sat_overlap(pos, tri, depth, 0.5 + delta)
    got = vu.grid_of(codes, depth)
    band = int((may & ~must).sum())
    print(f"{name}: delta {delta:.3g} voxel, leaves {len(codes)}, must {int(must.sum())}, may {int(may.sum())}, band {band}")
    assert not np.any(must & ~may)
    assert band <= 0.02 * may.sum(), (band, int(may.sum()))
    assert len(codes) > 1000 and must.sum() > 1000
    assert not np.any(must & ~got), int((must & ~got).sum())
    assert not np.any(got & ~may), int((got & ~may).sum())
    # the same condition at the issue's delta = 1e-3
    wide = int((vu.sat_overlap(pos, tri, depth, 0.5 + 1e-3) & ~vu.sat_overlap(pos, tri, depth, 0.5 - 1e-3)).sum())
    assert band <= wide <= 0.02 * may.sum(), wide
    if name == "bigtiny":
        assert (owner == 0).sum() > len(codes) / 2   # the spanning triangle is most of the scene
        assert len(np.unique(owner)) > 1000           # and the small ones are there
    if name == "ico2":   # counter-clockwise seen from outside: the normals point away from the centre
        xyz = vz.leaf_xyz(codes).astype(np.float64) + 0.5
        out = xyz - np.array([0.5013, 0.4987, 0.5021]) * (1 << depth)
        assert np.all((vu.reference(name)[1] * out).sum(1) > 0)


# ------------------------------------------------------------------ 3b. 512^3: the banded reference
@pytest.mark.parametrize("name", vu.MAIN + vu.MORE + vu.EDGES)
def test_band_reference_equals_reference(name):
    """What licenses the band: on every mesh that fits a dense grid, the rule evaluated on the band of each
    triangle's plane alone (large boxes, by Tri) or by the array form of Tri (small boxes) gives voxelize.voxelize's
    leaves, owners, normals, colours and statistics byte for byte."""
    variants = [(True, False)] + ([(False, True)] if name in ("ico2", "all_edges", "bigtiny") else [])
    for colors, flip in variants:
        want, got = vu.reference(name, colors, flip), vu.band_reference(name, colors, flip)
        same_leaves(got, want, name)
        assert got[4] == want[4], name
        assert all(a.dtype == b.dtype and a.shape == b.shape for a, b in zip(got[:4], want[:4]) if b is not None)
    cand = vu.batch_of(name).candidates()
    if name == "bigtiny":   # both paths: the spanning triangle's band through Tri, the 2,000 small boxes as arrays
        assert cand[0] > vu.SMALL_BOX and np.all(cand[1:] <= vu.SMALL_BOX) and np.all(cand[1:] > 0)
        t = vz.Tri(vu.mesh(name)[0][:3], 64)
        assert len(vu.band_cells(t, 64)) < 0.2 * t.candidates()   # and the band does prune
    tris = vz.setup(*vu.mesh(name)) if name in ("soup", "all_edges") else []
    assert [t.candidates() for t in tris] == cand[:len(tris)].tolist()


def test_span9_crosses_the_launch_limit_inside_a_triangle():
    """The conditions span9 is built for, from the rule's boxes alone: its four spanning triangles hold more than
    2^28 candidates (three do not), and candidate 2^28 of the only slab lies strictly inside one triangle's range,
    so the default launch limit ends one launch and starts the next in the middle of a box."""
    pos, tri, depth = vu.mesh("span9")
    assert depth == 9 and len(tri) == 2006 and list(vu.SPAN9_NAMED.values()) == [0, 2004, 2005]
    cand = vu.batch_of("span9").candidates()
    for k in (0, 1, 2, 3, 2004, 2005):
        assert vz.Tri(pos[tri[k]], 512).candidates() == cand[k]
    assert cand[:4].sum() > 2 ** 28 > cand[:3].sum() and 2.9e8 < cand[:4].sum() < 3.1e8
    ends = np.cumsum(cand)
    k = int(np.searchsorted(ends, 2 ** 28, side="right"))
    assert k == 3 and ends[k] - cand[k] < 2 ** 28 < ends[k] - 1
    assert 2 ** 28 < ends[-1] < 2 * 2 ** 28            # two launches at the default limit
    assert 512 * 512 * 512 * 4 == 512 << 20            # one slab at the default cell_bytes


@pytest.fixture(scope="module")
def span9_named():
    """Per named triangle of span9 at 512^3: (Tri, band cells, the rule on them, delta)."""
    pos, tri, depth = vu.mesh("span9_named")
    out = {}
    for k, name in enumerate(vu.SPAN9_NAMED):
        t = vz.Tri(pos[tri[k]], 1 << depth)
        cells = vu.band_cells(t, 1 << depth)
        out[name] = (t, cells, t.overlaps_at(cells), vu.rule_delta(pos, tri[k:k + 1], depth))
    return out


@pytest.mark.parametrize("name", list(vu.SPAN9_NAMED))
def test_rule_brackets_the_float64_overlap_at_512(span9_named, name):
    """must <= leaves <= may at 512^3, where delta is ten times what a 64^3 grid can show.  The float64 model is
    evaluated on the band: outside it a voxel is a whole cell away from every crossing of the plane with its
    column, which no cube of half extent below 1 reaches; the ring of one more cell around the band is evaluated
    too and holds no voxel of `may`.  The sliver's bracket holds but says little: its delta of a quarter voxel
    leaves more voxels undecided than it has leaves, so it is asserted without the 1 % cap."""
    t, cells, ok, delta = span9_named[name]
    n = 512
    v = t.v.astype(np.float64)
    key = lambda c: (c[:, 2] * n + c[:, 1]) * n + c[:, 0]
    assert len(np.unique(key(cells))) == len(cells)
    if name == "near_planar":   # its box is one voxel thick: the band is the box
        assert len(cells) == t.candidates() and t.bhi[1] == t.blo[1]
    else:
        assert len(cells) < 0.05 * t.candidates()
    grown = vu.band_cells(t, n, grow=1)
    ring = grown[~np.isin(key(grown), key(cells))]
    in_box = np.all((ring >= t.blo) & (ring <= t.bhi), axis=1)
    assert len(ring) > len(cells) / 4 and (in_box.sum() > 1000) == (name != "near_planar")
    assert not np.any(vu.sat_at(v, ring[in_box] + 0.5, 0.5 + delta))
    must, may = vu.sat_at(v, cells + 0.5, 0.5 - delta), vu.sat_at(v, cells + 0.5, 0.5 + delta)
    undecided = int((may & ~must).sum())
    print(f"{name}: delta {delta:.3g} voxel, candidates {t.candidates()}, band {len(cells)}, leaves {int(ok.sum())}, "
          f"must {int(must.sum())}, may {int(may.sum())}, undecided {undecided}")
    assert 0 < delta < 0.5 and ok.sum() > 1000
    assert not np.any(must & ~may)
    assert not np.any(must & ~ok), int((must & ~ok).sum())
    assert not np.any(ok & ~may), int((ok & ~may).sum())
    if name == "sliver":
        assert delta > 0.1    # on record: a spanning sliver's bound is weak
    else:
        assert delta < 1e-3 and undecided <= 0.01 * ok.sum(), (undecided, int(ok.sum()))


def test_header_equals_band_reference_at_512(driver):
    """The header through g++ on span9's three named triangles at 512^3 -- whole boxes, 1.9e8 candidates, nothing
    pruned -- gives the banded numpy reference byte for byte: no leaf of the rule lies outside the band, and the
    coordinates beyond 6 bits, the owners, normals, colours and statistics agree."""
    pos, tri, depth = vu.mesh("span9_named")
    want = vu.band_reference("span9_named")
    got = run_driver(driver, pos, tri, depth, vu.vertex_colors(pos))
    same_leaves(got, want, "span9_named")
    assert got[4] == want[4] and want[4]["candidates"] > 1.9e8
    assert set(want[3].tolist()) == {0, 1, 2} and vz.leaf_xyz(want[0]).max() >= 500


# ------------------------------------------------------------------ 4. owner and attribute rules
def test_owner_is_the_lowest_index_whatever_the_order():
    pos, tri, depth = vu.mesh("soup")
    codes, nrm, _, owner, _ = vu.reference("soup", colors=False)
    rev = vz.voxelize(pos, tri[::-1], depth)
    assert np.array_equal(rev[0], codes)                      # the voxel set does not change at all
    back = np.uint32(len(tri) - 1) - rev[3]                   # the reversed run's owners in the first run's numbering
    tris = vz.setup(pos, tri, depth)
    count = np.zeros(1 << (3 * depth), np.uint16)             # triangles per voxel, by Morton code
    for t in tris:
        if t.skipped:
            continue
        z, y, x = np.nonzero(t.overlaps())
        np.add.at(count, builder.morton(np.stack([x + t.blo[0], y + t.blo[1], z + t.blo[2]], 1)).astype(np.int64), 1)
    shared = count[codes.astype(np.int64)] > 1
    assert shared.sum() > 50 and (~shared).sum() > 1000
    assert np.array_equal(back[~shared], owner[~shared])      # one triangle: the same owner
    assert np.all(back[shared] > owner[shared])               # several: the lowest index here, the highest there
    assert rev[1][~shared].tobytes() == nrm[~shared].tobytes()


def test_flip_negates_every_normal_exactly():
    for name in ("ico2", "soup"):
        a, b = vu.reference(name, colors=False), vu.reference(name, colors=False, flip=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
        assert (a[1].view(np.uint32) ^ np.uint32(0x80000000)).tobytes() == b[1].tobytes()
        mag = np.linalg.norm(a[1].astype(np.float64), axis=1)
        assert np.all(np.abs(mag - 1) < 1e-6)


def test_colours_at_the_vertices_of_an_isolated_triangle():
    """Vertices on voxel centres: the leaf under vertex k takes vertex k's colour.  The weights there are 1 and 0
    up to the roundings of the stated order: w1, w2 carry 4 u (1 + kappa) each from the two cross products, the dot
    and D, w0 and the renormalisation two more; 64 u covers kappa <= 7 (this triangle's is below 3)."""
    depth, n = 5, 32
    centres = np.array([(5, 7, 9), (21, 10, 12), (11, 25, 17)], float)
    pos = ((centres + 0.5) / n).astype(f32)
    col = np.array([(1.0, 0.25, 0.0), (0.0, 1.0, 0.5), (0.125, 0.0, 1.0)], f32)
    codes, _, leafcol, owner = vz.voxelize(pos, [(0, 1, 2)], depth, colors=col)
    assert np.all(owner == 0) and len(codes) > 100
    xyz = vz.leaf_xyz(codes)
    for k in range(3):
        at = np.flatnonzero(np.all(xyz == centres[k].astype(np.uint32), axis=1))
        assert len(at) == 1
        assert np.all(np.abs(leafcol[at[0]].astype(np.float64) - col[k]) <= 64 * vu.U), (k, leafcol[at[0]])
    # every leaf colour is a convex combination of the three
    assert np.all(leafcol >= 0) and np.all(leafcol <= 1 + 4 * vu.U)
    # and in the middle: the centroid's voxel centre, against float64 barycentrics of its projection
    g = pos.astype(np.float64) * n
    N = np.cross(g[1] - g[0], g[2] - g[0])
    c = xyz.astype(np.float64) + 0.5
    q = c - g[0]
    w1 = np.cross(q, g[2] - g[0]) @ N / (N @ N)
    w2 = np.cross(g[1] - g[0], q) @ N / (N @ N)
    inside = (w1 > 0.05) & (w2 > 0.05) & (1 - w1 - w2 > 0.05)
    assert inside.sum() > 20
    want = (1 - w1 - w2)[:, None] * col[0] + w1[:, None] * col[1] + w2[:, None] * col[2]
    assert np.all(np.abs(leafcol[inside] - want[inside]) < 1e-5)


def test_fit_mesh():
    rng = np.random.default_rng(3)
    p = rng.uniform(-7, 20, (50, 3)) * (1, 0.5, 0.25)
    assert vz.fit_mesh(p, 0.1).dtype == f32
    q = vz.fit_mesh(p, 0.1).astype(np.float64)
    assert abs(q[:, 0].min() - 0.1) < 1e-6 and abs(q[:, 0].max() - 0.9) < 1e-6   # the longest axis fills the room
    assert np.allclose((q.max(0) + q.min(0)) / 2, 0.5, atol=1e-6)
    ratio = (q.max(0) - q.min(0)) / (p.max(0) - p.min(0))
    assert np.allclose(ratio, ratio[0])                                            # one scale
    with pytest.raises(ValueError):
        vz.fit_mesh(p, 0.5)


# ------------------------------------------------------------------ 5. watertight, end to end on the CPU
def test_ico2_pool_is_watertight(oracle_mod):
    """The ico2 leaves laid out by the numpy builder and traced by the oracle: a ray from outside the sphere toward
    a point inside it always hits, within sqrt(3) voxels of the sphere of radius 0.4 n."""
    pos, tri, depth = vu.mesh("ico2")
    codes, nrm, _, _, _ = vu.reference("ico2", colors=False)
    n = 1 << depth
    svo = builder.build_from_leaves(depth, vz.leaf_xyz(codes), nrm)
    osvo = qu.oracle_svo(oracle_mod, svo)
    rng = np.random.default_rng(53)
    centre = (np.array([0.5013, 0.4987, 0.5021]) - 0.5) * 32.0        # world: the cube is [-16, 16]^3
    radius = 0.4 * 32.0
    d = rng.normal(size=(2000, 3))
    origins = centre + 30.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    inner = rng.normal(size=(2000, 3))
    inner = centre + inner / np.linalg.norm(inner, axis=1, keepdims=True) * radius * 0.95 * rng.uniform(0, 1, (2000, 1)) ** (1 / 3)
    dirs = inner - origins
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rays = make_rays(origins.astype(f32), dirs.astype(f32))
    hits, _, _ = qu.oracle_trace(oracle_mod, osvo, rays)
    assert np.all(hits["flags"] & 1), int(np.count_nonzero((hits["flags"] & 1) == 0))
    o, dd = rays["origin"].astype(np.float64), rays["dir"].astype(np.float64)
    at = o + dd * (hits["t"].astype(np.float64) / 64.0)[:, None]     # t / 64 is the world ray's parameter
    dist = np.abs(np.linalg.norm(at - centre, axis=1) - radius) * (n / 32.0)   # in voxels
    print(f"watertight: worst distance from the sphere {dist.max():.3f} voxel")
    assert dist.max() <= 3 ** 0.5, dist.max()
